"""numpy restatement of the tetrahedron trace of the Green's function (helper of test_ltm_green_cpu.py /
test_gpu_ltm_green.py, not a conftest).

    tr G(z) = w sum_{cells} sum_{d! simplices} sum_{bands} J[x_0 ... x_d](z),     w = 1 / (d! npt^d),

over the mesh of ltm_numpy.kuhn_simplices.  J[x_0 ... x_m](z) is the mean of 1 / (z - e) over a simplex inside which e is
linear with the sorted corner values x_0 <= ... <= x_m, i.e. over the normalised B-spline with those knots.  With
u_i = z - x_i (all with the imaginary part of z):

    m = 0:  J = 1 / u_0
    m = 1:  J = (log u_0 - log u_1) / (x_1 - x_0)        principal logs; both arguments lie in one open half plane
    m >= 2: J[x_0..x_m] = m / (m - 1) (u_0 J[x_0..x_{m-1}] - u_m J[x_1..x_m]) / (x_m - x_0)

The evaluation rule: a sub-range x_i..x_j of width x_j - x_i < RHO |z - mean| is summed by its Taylor series

    J = sum_k  m! k! / (m + k)!  h_k(delta) / ubar^(k+1),      delta_l = x_l - mean,  ubar = z - mean,

h_k the complete homogeneous symmetric polynomial, by H_l^(k) = H_(l-1)^(k) + delta_l H_l^(k-1), H_0^(k) = delta_0^k, until
(max |delta| / |ubar|)^k < eps; only wider sub-ranges recurse, so nothing is divided by a width below RHO |ubar|.  The series
is scaled by 1 / |ubar|, so that neither delta^k nor ubar^-(k+1) leaves the range of a double.  Width exactly 0 gives 1 / u.
Re ubar is the mean of the Re u_l = Re z - x_l and delta_l = Re ubar - Re u_l, not z - mean(x) and x_l - mean(x): close to a
corner the differences Re z - x_l are exact and small, so ubar carries a relative error of eps, where the rounding of mean(x),
eps |x|, would move 1 / ubar by eps |x| / |ubar|^2 -- of order one per simplex at |ubar| = 1e-8.
Im z < 0: the conjugate of the value at conj(z).
"""
import math

import numpy as np

import ltm_numpy as ln

RHO = 0.5
EPS = 2.0**-52
KMAX = 40  # never reached: max |delta| / |ubar| <= RHO m / (m + 1) <= 3/8, 37 terms


def _series(x, z):
    """Taylor series of J for the knots x [k, m+1] (any order) about their mean.  Rows whose terms have fallen below eps leave
    the loop (the arrays are compressed when half of them have)."""
    m = x.shape[1] - 1
    ure = z.real - x  # Re u_l; the mean and the delta_l come from these, see the module's docstring
    ubr = ure.mean(axis=1)
    ub = ubr + 1j * z.imag
    s = 1.0 / np.abs(ub)
    dl = (ubr[:, None] - ure) * s[:, None]
    q = np.conj(ub) * s  # 1 / (ubar / |ubar|)
    r = np.abs(dl).max(axis=1)
    out = q * s  # k = 0: h_0 = 1
    idx = np.arange(len(x))
    H = np.ones_like(dl)
    acc = q.copy()
    p = q.copy()
    c = 1.0
    rk = r.copy()
    k = 0
    while k < KMAX and len(idx):
        live = rk >= EPS
        if 2 * np.count_nonzero(live) <= len(idx):
            out[idx] = acc * s[idx]
            idx, dl, H, acc, p, q, rk, r = idx[live], dl[live], H[live], acc[live], p[live], q[live], rk[live], r[live]
            if not len(idx):
                break
        k += 1
        H[:, 0] = H[:, 0] * dl[:, 0]
        for l in range(1, m + 1):
            H[:, l] = H[:, l - 1] + dl[:, l] * H[:, l]
        c = c * k / (m + k)
        p = p * q
        acc = acc + (c * H[:, m]) * p
        rk = rk * r
    out[idx] = acc * s[idx]
    return out


def simplex_J(x, z):
    """J[x_0 .. x_m](z) of the sorted knots x [ns, m+1] at one complex z with Im z > 0, by the evaluation rule."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[None, :]
    z = complex(z)
    assert z.imag > 0.0
    M = x.shape[1] - 1
    u = z - x
    logs = np.log(u)

    def J(i, j, rows):
        """J[x_i .. x_j] of the simplices `rows`; only the rows that recurse reach the narrower sub-ranges."""
        m = j - i
        if m == 0:
            return 1.0 / u[rows, i]
        xr = x[rows, i:j + 1]
        w = xr[:, -1] - xr[:, 0]
        small = w < RHO * np.abs((z.real - xr).mean(axis=1) + 1j * z.imag)
        out = np.empty(len(rows), dtype=np.complex128)
        if np.any(small):
            out[small] = _series(xr[small], z)
            flat = small & (w == 0.0)
            out[flat] = 1.0 / u[rows[flat], i]
        if not np.all(small):
            wide = rows[~small]
            ww = w[~small]
            if m == 1:
                out[~small] = (logs[wide, i] - logs[wide, j]) / ww
            else:
                out[~small] = (m / (m - 1.0)) * (u[wide, i] * J(i, j - 1, wide) - u[wide, j] * J(i + 1, j, wide)) / ww
        return out

    return J(0, M, np.arange(len(x)))


def simplex_J_any(x, z):
    """simplex_J for Im z of either sign."""
    z = complex(z)
    return simplex_J(x, z) if z.imag > 0 else np.conj(simplex_J(x, z.conjugate()))


def green_trace(eig, zs, simplices=None):
    """tr G(z) [nz] of the eigenvalues eig [npt]*d + [n] (per unit cell, summed over bands).  Equal simplices (a symmetric
    grid has many) are evaluated once and counted."""
    eig = np.asarray(eig, dtype=np.float64)
    d = eig.ndim - 1
    e = ln.kuhn_simplices(eig) if simplices is None else simplices
    e, counts = np.unique(e, axis=0, return_counts=True)
    weight = 1.0 / (math.factorial(d) * float(np.prod(eig.shape[:-1])))
    zs = np.atleast_1d(np.asarray(zs, dtype=np.complex128))
    out = np.empty(len(zs), dtype=np.complex128)
    for i, z in enumerate(zs):
        J = simplex_J_any(e, z) * counts
        out[i] = complex(math.fsum(J.real), math.fsum(J.imag)) * weight
    return out


def plain_grid_dos(eig, E, eta):
    """The plain grid mean of -Im 1 / (E + i eta - e) / pi, summed over bands: what a periodic grid sum of the resolvent gives."""
    eig = np.asarray(eig, dtype=np.float64)
    nk = float(np.prod(eig.shape[:-1]))
    return float(-(1.0 / (E + 1j * eta - eig)).imag.sum() / (math.pi * nk))


# ---------------------------------------------------------------- 60-digit reference
def mp_simplex_J(x, z, dps=60):
    """The pure recursion at `dps` digits for one simplex with sorted knots x; a sub-range of exactly zero width gives 1 / u."""
    import mpmath as mp
    with mp.workdps(dps):
        xs = [mp.mpf(float(v)) for v in x]
        zz = mp.mpc(complex(z).real, complex(z).imag)
        memo = {}

        def J(i, j):
            if (i, j) in memo:
                return memo[(i, j)]
            w = xs[j] - xs[i]
            if w == 0:
                out = 1 / (zz - xs[i])
            elif j - i == 1:
                out = (mp.log(zz - xs[i]) - mp.log(zz - xs[j])) / w
            else:
                m = j - i
                out = mp.mpf(m) / (m - 1) * ((zz - xs[i]) * J(i, j - 1) - (zz - xs[j]) * J(i + 1, j)) / w
            memo[(i, j)] = out
            return out

        v = J(0, len(xs) - 1)
        return v


def worst_relative_error(e, z):
    """max over the distinct simplices e [ns, m+1] of |J - J_mp| / |J_mp| at one z, in units of eps."""
    import mpmath as mp
    e = np.unique(np.asarray(e, dtype=np.float64), axis=0)
    J = simplex_J_any(e, z)
    worst = 0.0
    with mp.workdps(60):
        for row, v in zip(e, J):
            ref = mp_simplex_J(row, z)
            err = abs(mp.mpc(v.real, v.imag) - ref) / abs(ref)
            worst = max(worst, float(err))
    return worst / EPS

"""numpy restatement of the tetrahedron Green's function with matrix elements (helper of test_ltm_green_weighted_cpu.py /
test_gpu_ltm_green_weighted.py, not a conftest).

    G_A,c(z) = w sum_{cells} sum_{d! simplices} sum_{bands} sum_{i=0..m} A_{c,i} W_i(z),     w = 1 / (d! npt^d),  m = d,

over the mesh of ltm_numpy.kuhn_simplices, the element A_c linear inside a simplex like the energy.  W_i is the mean of
lambda_i / (z - e) over the simplex.  The uniform density on the simplex times lambda_i, normalised, is Dirichlet(1, .., 2, .., 1),
and its image under e is the B-spline with the knot x_i repeated, so with the sorted corner values x_0 <= ... <= x_m

    W_i = J[x_0 .. x_m, x_i](z) / (m + 1),

J the function of gltm_numpy.simplex_J, which takes knots with repeats as they are: its recursion holds for them with
J[x, x] = 1 / u (a sub-range of zero width), and its Taylor series for narrow sub-ranges takes any number of knots.  With five
knots (m = 3) max |delta| <= 4/5 width < 2/5 |ubar|: at most 39 terms, within gltm_numpy.KMAX.
Consequences checked in the tests: sum_i W_i = J[x_0 .. x_m] and sum_i x_i W_i = z J - 1.
Im z < 0: the conjugate of the value at conj(z) (the elements are real).
"""
import math

import numpy as np

import gltm_numpy as gn
from wltm_numpy import corner_sets


def simplex_weights(x, z):
    """W [ns, m+1] of the sorted knots x [ns, m+1] at one complex z with Im z > 0."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[None, :]
    ns, m1 = x.shape
    # the m + 1 multisets of every simplex, x_i doubled and still sorted, in one call: rows [i ns, (i + 1) ns) double knot i
    y = np.concatenate([np.concatenate([x[:, :i + 1], x[:, i:]], axis=1) for i in range(m1)], axis=0)
    return gn.simplex_J(y, z).reshape(m1, ns).T / m1


def simplex_weights_any(x, z):
    """simplex_weights for Im z of either sign."""
    z = complex(z)
    return simplex_weights(x, z) if z.imag > 0 else np.conj(simplex_weights(x, z.conjugate()))


def sorted_corners(eig, A):
    """eig [npt]*d + [n], A [ncomp] + eig.shape -> (e [S, d+1] ascending, a [S, d+1, ncomp]) of every (permutation, cell, band),
    the elements carried along with the energies."""
    eig = np.asarray(eig, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    if A.shape == eig.shape:
        A = A[None]
    assert A.shape[1:] == eig.shape, (A.shape, eig.shape)
    d = eig.ndim - 1
    ncomp = A.shape[0]
    ce = corner_sets(eig, d).transpose(0, 2, 1).reshape(-1, d + 1)
    cA = corner_sets(np.moveaxis(A, 0, -1), d).transpose(0, 2, 1, 3).reshape(-1, d + 1, ncomp)
    o = np.argsort(ce, axis=1, kind="stable")
    return np.take_along_axis(ce, o, 1), np.take_along_axis(cA, o[:, :, None], 1)


def green_weighted(eig, A, zs):
    """G_A(z) [nz, ncomp] of the eigenvalues eig [npt]*d + [n] and the elements A [ncomp] + eig.shape (per unit cell, summed over
    bands).  Equal (simplex, elements) rows are evaluated once and counted."""
    eig = np.asarray(eig, dtype=np.float64)
    d = eig.ndim - 1
    e, a = sorted_corners(eig, A)
    ncomp = a.shape[2]
    rows, counts = np.unique(np.concatenate([e, a.reshape(len(e), -1)], axis=1), axis=0, return_counts=True)
    e, a = rows[:, :d + 1], rows[:, d + 1:].reshape(-1, d + 1, ncomp)
    weight = 1.0 / (math.factorial(d) * float(np.prod(eig.shape[:-1])))
    zs = np.atleast_1d(np.asarray(zs, dtype=np.complex128))
    out = np.empty((len(zs), ncomp), dtype=np.complex128)
    for i, z in enumerate(zs):
        W = simplex_weights_any(e, z) * counts[:, None]
        for c in range(ncomp):
            t = (a[:, :, c] * W).ravel()
            out[i, c] = complex(math.fsum(t.real), math.fsum(t.imag)) * weight
    return out


# ---------------------------------------------------------------- multi-precision reference
# The pure recursion loses log10(|u| / width) digits at every level, and the eigenvalues of a grid have corners an ulp apart
# (width 2e-16 |x|: graphene at 12 points has the triangle (1 - 1.9e-15, 1 - 2.2e-16, 1)).  The trace of that triangle has two
# levels, 2 x 16 digits, and its test's 60 digits survive; the doubled triangle has three and the doubled tetrahedron four: at
# 60 digits the REFERENCE was off by up to 7e4 eps on such simplices at |u| = 4 (at 130 digits the restatement is 0.6 eps from
# it).  130 digits leave more than 60 correct after four levels of 1e16.
MP_DPS = 130


def mp_simplex_weights(x, z, dps=MP_DPS):
    """The pure recursion at `dps` digits for the m + 1 doubled-knot multisets of one simplex with sorted knots x; a sub-range
    of exactly zero width gives 1 / u.  The multisets share their sub-ranges: one memo, keyed by the knots."""
    import mpmath as mp
    with mp.workdps(dps):
        xs = [mp.mpf(float(v)) for v in x]
        zz = mp.mpc(complex(z).real, complex(z).imag)
        logs = [mp.log(zz - v) for v in xs]
        memo = {}

        def J(k):  # k: ascending indices into xs, one of them possibly twice
            if k in memo:
                return memo[k]
            i, j = k[0], k[-1]
            w = xs[j] - xs[i]
            if w == 0:
                out = 1 / (zz - xs[i])
            elif len(k) == 2:
                out = (logs[i] - logs[j]) / w
            else:
                M = len(k) - 1
                out = mp.mpf(M) / (M - 1) * ((zz - xs[i]) * J(k[:-1]) - (zz - xs[j]) * J(k[1:])) / w
            memo[k] = out
            return out

        idx = tuple(range(len(xs)))
        return [J(idx[:i + 1] + idx[i:]) / len(xs) for i in range(len(xs))]


def worst_weight_error(e, z):
    """max over the distinct simplices e [ns, m+1] of max_i |W_i - W_i,mp| / max_i |W_i,mp| at one z, in units of eps, and the
    simplex that shows it."""
    import mpmath as mp
    e = np.unique(np.asarray(e, dtype=np.float64), axis=0)
    W = simplex_weights_any(e, z)
    worst, where = 0.0, None
    with mp.workdps(MP_DPS):
        for row, w in zip(e, W):
            ref = mp_simplex_weights(row, z)
            scale = max(abs(r) for r in ref)
            err = max(abs(mp.mpc(v.real, v.imag) - r) for v, r in zip(w, ref)) / scale
            if float(err) > worst:
                worst, where = float(err), row.copy()
    return worst / gn.EPS, where

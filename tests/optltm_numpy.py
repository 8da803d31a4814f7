"""numpy restatement of the optimized tetrahedron method (helper of test_ltm_optimized_cpu.py / test_gpu_ltm_optimized.py,
not a conftest).

Kawamura, Gohda, Tsuneyuki, PRB 89, 094515 (2014), d = 3.  A Kuhn simplex of cell i is the path v1 = i, v2 = v1 + e_a,
v3 = v2 + e_b, v4 = v3 + e_c over a permutation (a, b, c) of the axes.  The band is taken at 20 grid points,

    p1..p4   = v1..v4
    p5..p16  = 2 v_i - v_j,  (i, j) = (1,2) (2,3) (3,4) (4,1) (1,3) (2,4) (3,1) (4,2) (1,4) (2,1) (3,2) (4,3)
    p17..p20 = v4 - v1 + v2,  v1 - v2 + v3,  v2 - v3 + v4,  v3 - v4 + v1

(every index mod npt), the cubic through the 20 values is fitted, and the 4 corner values are replaced by those of the
linear function closest to the cubic in the least-squares sense over the simplex: x'_m = sum_j P[m][j] x(p_j).  The
closed forms of the linear method then apply to (e'_1..e'_4; A'_1..A'_4).

`projection()` derives P from that definition in exact rationals; nothing here holds the table.  The sums are the
closed-form corner weights of Bloechl, Jepsen, Andersen, PRB 49, 16223 (1994), written for any float type so that the
f64 evaluation can be set against a longdouble one; test_ltm_optimized_cpu.py sets them against the geometric
restatement of wltm_numpy.py on plain corners.
"""
import itertools
import math
from fractions import Fraction

import numpy as np

PAIRS = ((1, 2), (2, 3), (3, 4), (4, 1), (1, 3), (2, 4), (3, 1), (4, 2), (1, 4), (2, 1), (3, 2), (4, 3))
# p17..p20 as (plus, minus, plus)
TRIPLES = ((4, 1, 2), (1, 2, 3), (2, 3, 4), (3, 4, 1))


def points(perm=(0, 1, 2)):
    """The 20 points of the simplex of the path `perm` as integer offsets [20, 3] from the cell's corner 0."""
    v = [np.zeros(3, dtype=int)]
    for ax in perm:
        nxt = v[-1].copy()
        nxt[ax] += 1
        v.append(nxt)
    p = list(v)
    p += [2 * v[i - 1] - v[j - 1] for i, j in PAIRS]
    p += [v[a - 1] - v[b - 1] + v[c - 1] for a, b, c in TRIPLES]
    return np.array(p)


def barycentric(perm=(0, 1, 2)):
    """The 20 points in the simplex's own coordinates (u, v, w): p = v1 + u (v2 - v1) + v (v3 - v1) + w (v4 - v1), as
    Fractions [20][3].  The simplex is u, v, w >= 0, u + v + w <= 1."""
    a, b, c = perm
    out = []
    for p in points(perm):
        al, be, ga = int(p[a]), int(p[b]), int(p[c])  # p = v1 + al e_a + be e_b + ga e_c
        out.append((Fraction(al - be), Fraction(be - ga), Fraction(ga)))
    return out


MONOMIALS = [(i, j, k) for i in range(4) for j in range(4) for k in range(4) if i + j + k <= 3]


def moment(i, j, k):
    """int u^i v^j w^k over the simplex u, v, w >= 0, u + v + w <= 1"""
    return Fraction(math.factorial(i) * math.factorial(j) * math.factorial(k), math.factorial(i + j + k + 3))


def _solve(M, B):
    """M^-1 B in Fractions (Gauss-Jordan with row exchanges)."""
    n = len(M)
    A = [list(M[r]) + list(B[r]) for r in range(n)]
    for c in range(n):
        piv = next(r for r in range(c, n) if A[r][c] != 0)
        A[c], A[piv] = A[piv], A[c]
        inv = 1 / A[c][c]
        A[c] = [x * inv for x in A[c]]
        for r in range(n):
            if r != c and A[r][c] != 0:
                f = A[r][c]
                A[r] = [x - f * y for x, y in zip(A[r], A[c])]
    return [row[n:] for row in A]


def cubic_coefficients():
    """C [20 monomials][20 points]: the coefficients of the cubic through the values at the 20 points."""
    pts = barycentric()
    M = [[u ** i * v ** j * w ** k for (i, j, k) in MONOMIALS] for (u, v, w) in pts]
    I = [[Fraction(int(r == c)) for c in range(20)] for r in range(20)]
    return _solve(M, I)


# lambda_m of the corner m as coefficients of (1, u, v, w)
LAMBDA = ((1, -1, -1, -1), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1))
_UNIT = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))


def _lambda_moment(m, mono):
    """int lambda_m u^i v^j w^k over the simplex"""
    i, j, k = mono
    return sum(c * moment(i + du, j + dv, k + dw) for c, (du, dv, dw) in zip(LAMBDA[m], _UNIT))


def gram():
    """G [4][4] = int lambda_m lambda_n"""
    G = [[Fraction(0)] * 4 for _ in range(4)]
    for m in range(4):
        for n in range(4):
            G[m][n] = sum(cn * _lambda_moment(m, mono) for cn, mono in zip(LAMBDA[n], _UNIT))
    return G


def projection():
    """P [4][20] in Fractions: the corner values of the linear function that minimises int (cubic - linear)^2."""
    C = cubic_coefficients()
    B = [[sum(_lambda_moment(m, mono) * C[q][j] for q, mono in enumerate(MONOMIALS)) for j in range(20)] for m in range(4)]
    return _solve(gram(), B)


_P64 = None


def projection_float(dtype=np.float64):
    global _P64
    if _P64 is None:
        _P64 = projection()
    return np.array([[dtype(x.numerator) / dtype(x.denominator) for x in row] for row in _P64], dtype=dtype)


def stencil_values(arr, perm):
    """arr [npt, npt, npt, ...] -> [20, ncell, ...]: the values at the 20 points of the simplex `perm` of every cell."""
    out = []
    for off in points(perm):
        cur = arr
        for ax in range(3):
            if off[ax]:
                cur = np.roll(cur, -int(off[ax]), axis=ax)  # the value at i + off, wrapped
        out.append(cur.reshape((-1,) + arr.shape[3:]))
    return np.stack(out)


def effective_corners(arr, dtype=np.float64, optimized=True):
    """arr [npt]*3 + [...] -> [6 ncell, 4, ...]: the effective corner values x' of every (permutation, cell); with
    optimized=False the 4 corner values themselves."""
    P = projection_float(dtype)
    arr = np.asarray(arr, dtype=dtype)
    out = []
    for perm in itertools.permutations(range(3)):
        x = stencil_values(arr, perm)
        out.append(np.tensordot(P, x, axes=(1, 0)) if optimized else x[:4])
    return np.concatenate([np.moveaxis(o, 0, 1) for o in out], axis=0)


def _weights(e, E, states):
    """Corner weights [K, 4] of simplices with sorted corner energies e [K, 4], all with e1 <= E < e4; unit = one simplex."""
    one = e.dtype.type(1)
    e1, e2, e3, e4 = e.T
    w = np.zeros_like(e)
    with np.errstate(divide="ignore", invalid="ignore"):
        r1 = E < e2
        r3 = ~r1 & ~(E < e3)
        r2 = ~r1 & ~r3
        # e1 <= E < e2
        t2, t3, t4 = (E - e1) / (e2 - e1), (E - e1) / (e3 - e1), (E - e1) / (e4 - e1)
        q = t2 * t3 * t4 / 4 if states else t3 * t4 / (e2 - e1)
        a = np.stack([(4 if states else 3) * q - q * (t2 + t3 + t4), q * t2, q * t3, q * t4], axis=1)
        # e3 <= E < e4: the mirror image from corner 4
        s1, s2, s3 = (e4 - E) / (e4 - e1), (e4 - E) / (e4 - e2), (e4 - E) / (e4 - e3)
        q = s1 * s2 * s3 / 4 if states else s1 * s2 / (e4 - e3)
        c = np.stack([q * s1, q * s2, q * s3, (4 if states else 3) * q - q * (s1 + s2 + s3)], axis=1)
        if states:
            c = one / 4 - c
        # e2 <= E < e3: the prism below E cut into three tetrahedra, the cut into two triangles
        t13, t14, t23, t24 = (E - e1) / (e3 - e1), (E - e1) / (e4 - e1), (E - e2) / (e3 - e2), (E - e2) / (e4 - e2)
        if states:
            v1, v2, v3 = t13 * t14 / 4, t14 * t23 * (1 - t13) / 4, (1 - t14) * t23 * t24 / 4
            p13, p14, p23, p24, c1, c2 = v1 + v2, v1 + v2 + v3, v2 + v3, v3, v1, v1 + v2 + v3
        else:
            ga, gb = t13 * (1 - t23) / (e4 - e1), t23 * (1 - t24) / (e4 - e1)
            p13, p14, p23, p24, c1, c2 = ga, ga + gb, ga + gb, gb, 0, 0
        b = np.stack([c1 + p13 * (1 - t13) + p14 * (1 - t14), c2 + p23 * (1 - t23) + p24 * (1 - t24), p13 * t13 + p23 * t23,
                      p14 * t14 + p24 * t24], axis=1)
    w[r1] = a[r1]
    w[r2] = b[r2]
    w[r3] = c[r3]
    return w


def _total(x):
    """column sums of x [K, ncomp]: exact for f64, in the array's own type otherwise"""
    if x.dtype == np.float64:
        return np.array([math.fsum(col) for col in x.T.tolist()])
    return x.sum(axis=0)


def simplex_sums(ce, cA, Es, states):
    """Corner energies ce [S, 4] and elements cA [S, 4, ncomp] of S simplices (any order of the corners) -> [nE, ncomp]:
    the sum over the simplices of g_A (or N_A with `states`), unit = one simplex.  Half-open regions e_i <= E < e_{i+1}; a
    simplex wholly below E gives the mean of its A to N_A, a flat one nothing to g_A."""
    o = np.argsort(ce, axis=1, kind="stable")
    ce = np.take_along_axis(ce, o, 1)
    cA = np.take_along_axis(cA, o[:, :, None], 1)
    lo, hi = ce[:, 0], ce[:, -1]
    out = np.zeros((len(Es), cA.shape[2]), dtype=ce.dtype)
    for i, E in enumerate(np.asarray(Es, dtype=ce.dtype)):
        inside = (lo <= E) & (E < hi)
        tot = np.zeros(cA.shape[2], dtype=ce.dtype)
        if inside.any():
            w = _weights(ce[inside], E, states)
            tot = tot + _total(np.einsum("kv,kvc->kc", w, cA[inside]))
        if states:
            below = hi <= E
            if below.any():
                tot = tot + _total(cA[below].mean(axis=1))
        out[i] = tot
    return out


def optltm(eig, A, Es, states, dtype=np.float64, optimized=True):
    """eig [npt]*3 + [n] ascending eigenvalues, A None (A = 1), "energy" (A = e) or [ncomp] + eig.shape, energies Es ->
    g_A or N_A [nE, ncomp] of the optimized rule, per unit cell and summed over bands (optimized=False: of the linear rule)."""
    eig = np.asarray(eig, dtype=dtype)
    n = eig.shape[-1]
    ce = effective_corners(eig, dtype, optimized)          # [S, 4, n]
    if A is None:
        cA = np.ones(ce.shape + (1,), dtype=dtype)
    elif isinstance(A, str):
        assert A == "energy"
        cA = ce[..., None]
    else:
        A = np.asarray(A, dtype=dtype)
        assert A.shape[1:] == eig.shape, (A.shape, eig.shape)
        cA = effective_corners(np.moveaxis(A, 0, -1), dtype, optimized)  # [S, 4, n, ncomp]
    ce = ce.transpose(0, 2, 1).reshape(-1, 4)
    cA = cA.transpose(0, 2, 1, 3).reshape(-1, 4, cA.shape[-1])
    w = dtype(1) / dtype(6 * eig.shape[0] * eig.shape[1] * eig.shape[2])
    return simplex_sums(ce, cA, np.atleast_1d(Es), states) * w


def issue_band(npt, dtype=np.float64):
    """e(k) = -2 sum_i cos 2 pi k_i + 0.5 cos 2 pi (k_1 + k_2) on the grid, [npt, npt, npt, 1]"""
    k = 2 * np.pi * np.arange(npt, dtype=dtype) / npt
    k1, k2, k3 = np.meshgrid(k, k, k, indexing="ij")
    return (-2 * (np.cos(k1) + np.cos(k2) + np.cos(k3)) + 0.5 * np.cos(k1 + k2))[..., None]

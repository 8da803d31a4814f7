"""numpy restatement of the linear tetrahedron method with matrix elements (helper of test_ltm_weighted_cpu.py /
test_gpu_ltm_weighted.py, not a conftest).

With A_b(k) per node and band, interpolated linearly inside every simplex like the band energy,

    g_A(E) = sum_b int A_b(k) delta(E - e_b(k)) dk,     N_A(E) = sum_b int A_b(k) theta(E - e_b(k)) dk.

This is a GEOMETRIC restatement, deliberately not the closed-form corner weights of kernels_ltm.hip: for every simplex
(the Kuhn split and the weights of ltm_numpy.py) it builds the sub-simplices that fill {e < E} and the simplices of the
cut {e = E} as matrices B of barycentric coordinates, one row per vertex, and uses only two facts:

* a linear function integrates over a simplex to volume x mean of its vertex values, and the volume of a sub-simplex
  is |det B| of the parent's:                       N_A += |det B| mean(B A);
* the cone from a corner (the apex) over a piece C of the cut has volume |det [C; apex]|, and moving the cut by dE
  thickens it by dE / |e_apex - E| of the apex's distance, d times the cone's volume per unit distance:
                                                    g_A += d |det [C; apex]| / |e_apex - E| mean(C A).
  The apex is the corner farthest from E in energy.

Sums over simplices: blocks of 16 are added by numpy, the block sums go through math.fsum (plain fsum over every
simplex and component made the 1500-energy GPU cases minutes long; a block sum is off by at most 15 roundings of its
own terms, 1.7e-15 of them, whatever the number of simplices).  Half-open regions e_i <= E < e_{i+1} as in ltm_numpy.py; a simplex wholly below E
gives mean(A), a flat one nothing to g_A.
"""
import itertools
import math

import numpy as np


def corner_sets(arr, d):
    """arr [npt]*d + [...] -> [nsimplex, d + 1, ...]: the corner values of every (permutation, cell)."""
    out = []
    for perm in itertools.permutations(range(d)):
        cs = [arr]
        cur = arr
        for ax in perm:
            cur = np.roll(cur, -1, axis=ax)
            cs.append(cur)
        out.append(np.stack([c.reshape((-1,) + arr.shape[d:]) for c in cs], axis=1))
    return np.concatenate(out, axis=0)


def _pieces(e, E):
    """Sorted corner energies e [K, d+1], all with the same number m of corners at or below E (1 <= m <= d).
    -> (below, complement, cut): lists of vertex matrices [K, d+1, d+1] filling {e < E} (or, with `complement`, the
    part ABOVE E instead), and of [K, d, d+1] filling the cut."""
    K, d1 = e.shape
    d = d1 - 1
    I = np.eye(d1)
    m = int(np.count_nonzero(e[0] <= E))

    def C(i):
        return np.broadcast_to(I[i], (K, d1))

    def P(i, j):  # the point of edge i-j with energy E
        t = ((E - e[:, i]) / (e[:, j] - e[:, i]))[:, None]
        return (1.0 - t) * I[i] + t * I[j]

    S = lambda *v: np.stack(v, axis=1)
    if d == 1:
        return [S(C(0), P(0, 1))], False, [S(P(0, 1))]
    if d == 2:
        if m == 1:
            return [S(C(0), P(0, 1), P(0, 2))], False, [S(P(0, 1), P(0, 2))]
        return [S(C(0), C(1), P(1, 2)), S(C(0), P(1, 2), P(0, 2))], False, [S(P(0, 2), P(1, 2))]
    if m == 1:
        return [S(C(0), P(0, 1), P(0, 2), P(0, 3))], False, [S(P(0, 1), P(0, 2), P(0, 3))]
    if m == 2:  # a prism: the triangle (0, P02, P03) swept to (1, P12, P13)
        a, b, c, a2, b2, c2 = C(0), P(0, 2), P(0, 3), C(1), P(1, 2), P(1, 3)
        return [S(a, b, c, a2), S(b, c, a2, b2), S(c, a2, b2, c2)], False, [S(b, c, b2), S(c, b2, c2)]
    return [S(P(0, 3), P(1, 3), P(2, 3), C(3))], True, [S(P(0, 3), P(1, 3), P(2, 3))]  # the tip at corner 3


def wltm(eig, A, Es):
    """eig [npt]*d + [n] ascending eigenvalues, A [ncomp] + eig.shape (or eig.shape: one component), energies Es
    -> (g_A, N_A), each [nE, ncomp], per unit cell and summed over bands."""
    eig = np.asarray(eig, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    if A.shape == eig.shape:
        A = A[None]
    assert A.shape[1:] == eig.shape, (A.shape, eig.shape)
    ncomp = A.shape[0]
    d = eig.ndim - 1
    d1 = d + 1
    ce = corner_sets(eig, d)                            # [ns, d+1, n]
    cA = corner_sets(np.moveaxis(A, 0, -1), d)          # [ns, d+1, n, ncomp]
    ce = ce.transpose(0, 2, 1).reshape(-1, d1)
    cA = cA.transpose(0, 2, 1, 3).reshape(-1, d1, ncomp)
    o = np.argsort(ce, axis=1, kind="stable")
    ce = np.take_along_axis(ce, o, 1)
    cA = np.take_along_axis(cA, o[:, :, None], 1)
    lo, hi = ce[:, 0], ce[:, -1]
    means = cA.mean(axis=1)                             # [S, ncomp]
    w = 1.0 / (math.factorial(d) * float(np.prod(eig.shape[:d])))
    Es = np.atleast_1d(np.asarray(Es, dtype=np.float64))
    g = np.zeros((len(Es), ncomp))
    N = np.zeros((len(Es), ncomp))

    def fs(x):  # column sums of x [K, ncomp]
        x = np.asarray(x)
        pad = (-len(x)) % 16
        if pad:
            x = np.concatenate([x, np.zeros((pad, x.shape[1]))])
        blocks = x.reshape(-1, 16, x.shape[1]).sum(axis=1)
        return [math.fsum(col) for col in blocks.T.tolist()]

    # simplices wholly below E, by ascending energy: what each energy adds to the one before it, then exact prefix sums
    by_hi = np.argsort(hi, kind="stable")
    hi_sorted = hi[by_hi]
    order = np.argsort(Es, kind="stable")
    steps = [[] for _ in range(ncomp)]
    prev = 0
    for i in order:
        E = Es[i]
        upto = int(np.searchsorted(hi_sorted, E, side="right"))  # hi <= E
        inc = fs(means[by_hi[prev:upto]]) if upto > prev else [0.0] * ncomp
        prev = max(prev, upto)
        for c in range(ncomp):
            steps[c].append(inc[c])
        Nc = [[math.fsum(steps[c])] for c in range(ncomp)]
        gc = [[] for _ in range(ncomp)]
        inside = np.flatnonzero((lo <= E) & (E < hi))
        if len(inside):
            e_in, a_in = ce[inside], cA[inside]
            m_in = np.count_nonzero(e_in <= E, axis=1)
            for m in range(1, d1):
                sel = m_in == m
                if not sel.any():
                    continue
                e, a = e_in[sel], a_in[sel]
                below, complement, cut = _pieces(e, E)
                vmean = lambda B: np.einsum("kv,kvc->kc", B.mean(axis=1), a)  # mean over the vertices of B of (B A)
                part = sum(np.abs(np.linalg.det(B))[:, None] * vmean(B) for B in below)
                if complement:
                    part = a.mean(axis=1) - part
                apex = np.where((E - e[:, 0]) >= (e[:, -1] - E), 0, d)
                e_apex = np.take_along_axis(e, apex[:, None], 1)[:, 0]
                tip = np.eye(d1)[apex][:, None, :]
                dens = sum((d * np.abs(np.linalg.det(np.concatenate([Cm, tip], axis=1))) / np.abs(e_apex - E))[:, None] *
                           vmean(Cm) for Cm in cut)
                for c, col in enumerate(fs(part)):
                    Nc[c].append(col)
                for c, col in enumerate(fs(dens)):
                    gc[c].append(col)
        for c in range(ncomp):
            N[i, c] = math.fsum(Nc[c]) * w
            g[i, c] = math.fsum(gc[c]) * w
    return g, N

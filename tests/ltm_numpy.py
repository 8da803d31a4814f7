"""numpy restatement of the linear tetrahedron method (helper of test_ltm_cpu.py / test_gpu_ltm.py, not a conftest).

Bloechl, Jepsen, Andersen, PRB 49, 16223 (1994), without the curvature correction; the reference has no LTM
(src/dos_algorithms.jl:1-7 plans it), so this is written from the paper's formulas:

* the periodic grid of npt^d nodes is cut into cells with corners i + {0,1}^d (indices mod npt), every cell into d!
  simplices by the Kuhn (Freudenthal) split: one per permutation of the axes, walking from corner 0 to corner (1..1);
* every simplex weighs 1 / (d! npt^d); band b of a simplex is the b-th ascending eigenvalue at each corner;
* sorted corner energies e1 <= ... <= e_{d+1}, e_ij = e_i - e_j, half-open regions e_i <= E < e_{i+1}.
"""
import itertools
import math

import numpy as np


def kuhn_simplices(eig):
    """eig [npt]*d + [n] ascending eigenvalues on the grid -> sorted corner energies [nsimplex, d + 1] of every
    (cell, permutation, band)."""
    eig = np.asarray(eig, dtype=np.float64)
    d = eig.ndim - 1
    out = []
    for perm in itertools.permutations(range(d)):
        corners = [eig]
        cur = eig
        for ax in perm:
            cur = np.roll(cur, -1, axis=ax)  # the neighbour at +1 along `ax`, wrapped
            corners.append(cur)
        out.append(np.stack([c.reshape(-1) for c in corners], axis=1))
    return np.sort(np.concatenate(out, axis=0), axis=1)


def _g(e, E):
    """DOS of simplices e [m, d+1], all with e1 <= E < e_last."""
    d = e.shape[1] - 1
    if d == 1:
        return 1.0 / (e[:, 1] - e[:, 0])
    if d == 2:
        e1, e2, e3 = e.T
        e21, e31, e32 = e2 - e1, e3 - e1, e3 - e2
        lo = E < e2
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(lo, 2 * (E - e1) / (e21 * e31), 2 * (e3 - E) / (e31 * e32))
    e1, e2, e3, e4 = e.T
    e21, e31, e41, e32, e42, e43 = e2 - e1, e3 - e1, e4 - e1, e3 - e2, e4 - e2, e4 - e3
    x = E - e2
    with np.errstate(divide="ignore", invalid="ignore"):
        r1 = 3 * (E - e1) ** 2 / (e21 * e31 * e41)
        r2 = (3 * e21 + 6 * x - 3 * (e31 + e42) * x**2 / (e32 * e42)) / (e31 * e41)
        r3 = 3 * (e4 - E) ** 2 / (e41 * e42 * e43)
    return np.where(E < e2, r1, np.where(E < e3, r2, r3))


def _n(e, E):
    """State count of simplices e [m, d+1], all with e1 <= E < e_last."""
    d = e.shape[1] - 1
    if d == 1:
        return (E - e[:, 0]) / (e[:, 1] - e[:, 0])
    if d == 2:
        e1, e2, e3 = e.T
        e21, e31, e32 = e2 - e1, e3 - e1, e3 - e2
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(E < e2, (E - e1) ** 2 / (e21 * e31), 1 - (e3 - E) ** 2 / (e31 * e32))
    e1, e2, e3, e4 = e.T
    e21, e31, e41, e32, e42, e43 = e2 - e1, e3 - e1, e4 - e1, e3 - e2, e4 - e2, e4 - e3
    x = E - e2
    with np.errstate(divide="ignore", invalid="ignore"):
        r1 = (E - e1) ** 3 / (e21 * e31 * e41)
        r2 = (e21**2 + 3 * e21 * x + 3 * x**2 - (e31 + e42) * x**3 / (e32 * e42)) / (e31 * e41)
        r3 = 1 - (e4 - E) ** 3 / (e41 * e42 * e43)
    return np.where(E < e2, r1, np.where(E < e3, r2, r3))


def ltm(eig, Es):
    """(g, N) at the energies Es: DOS and number of states below E, per unit cell, summed over bands
    (integral of g = n = N(+inf)).  A simplex wholly below E counts 1, a flat one contributes nothing to g."""
    eig = np.asarray(eig, dtype=np.float64)
    d = eig.ndim - 1
    e = kuhn_simplices(eig)
    lo, hi = e[:, 0], e[:, -1]
    weight = 1.0 / (math.factorial(d) * float(np.prod(eig.shape[:-1])))
    Es = np.atleast_1d(np.asarray(Es, dtype=np.float64))
    g = np.zeros(len(Es))
    N = np.zeros(len(Es))
    for i, E in enumerate(Es):
        inside = (lo <= E) & (E < hi)
        below = np.count_nonzero(hi <= E)
        ei = e[inside]
        if len(ei):
            g[i] = math.fsum(_g(ei, E)) * weight
            N[i] = (math.fsum(_n(ei, E)) + below) * weight
        else:
            N[i] = below * weight
    return g, N


def grid_eigenvalues(series, npt):
    """Ascending eigenvalues [npt]*d + [n] of an oracle FourierSeries on the PTR grid (numpy.linalg.eigvalsh)."""
    import abz_oracle as orc
    vals = np.asarray(orc.fourier_ptr(series, npt))
    d = series.d
    if vals.ndim == d:  # scalar series
        return vals.real[..., None]
    return np.linalg.eigvalsh(vals)


def rule_eigenvalues(rule):
    """The exported eigenvalues of a full-grid DeviceRule as [npt]*d + [n] (node index has i_1 fastest; the Kuhn split
    takes every permutation of the axes, so their order does not matter)."""
    E = rule.export(x=False, w=False, eig=True)["eig"]
    d = rule.dev.s.d
    return E.reshape((rule.npt,) * d + (E.shape[1],))

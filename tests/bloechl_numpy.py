"""numpy restatement of Bloechl's curvature correction of the weighted state sum (helper of test_ltm_bloechl_cpu.py /
test_gpu_ltm_bloechl.py, not a conftest).

Bloechl, Jepsen, Andersen, PRB 49, 16223 (1994), eq. 22, generalised to d = 1, 2, 3.  For a simplex T of a d-dimensional
grid with corner energies e_1 .. e_{d+1} and elements A_1 .. A_{d+1} (following the band index like the energies),

    N_A^corr(E) = N_A(E) + w sum_T g_T(E) kappa_T,   kappa_T = f_d sum_i A_i (sum_l e_l - (d+1) e_i),   f_d = 1 / (2 (d+1)(d+2)),

g_T the simplex's own DOS (ltm_numpy._g), w = 1 / (d! npt^d); only simplices with e_1 <= E < e_{d+1} contribute.  The
corners come from wltm_numpy.corner_sets, sorted stably with the elements carried along; sums over simplices are block
sums of 16 through math.fsum, as in wltm_numpy.  Nothing here is shared with the closed forms of kernels_ltm.hip
beyond the published g formulas.

The correction removes the leading O(1/npt^2) error of a sum taken at FIXED FILLING (E = the grid's own Fermi level);
at a fixed energy the misplaced Fermi surface leaves an error of the same order.
"""
import math

import numpy as np

import ltm_numpy as ln
import wltm_numpy as wn


def factor(d):
    return 1.0 / (2.0 * (d + 1) * (d + 2))


def _fs(x):
    """column sums of x [K, ncomp]: blocks of 16 by numpy, the block sums by math.fsum"""
    x = np.asarray(x)
    pad = (-len(x)) % 16
    if pad:
        x = np.concatenate([x, np.zeros((pad, x.shape[1]))])
    blocks = x.reshape(-1, 16, x.shape[1]).sum(axis=1)
    return [math.fsum(col) for col in blocks.T.tolist()]


def sorted_simplices(eig, A):
    """eig [npt]*d + [n], A [ncomp] + eig.shape -> (e [S, d+1] ascending, a [S, d+1, ncomp] carried along, weight)"""
    eig = np.asarray(eig, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    if A.shape == eig.shape:
        A = A[None]
    assert A.shape[1:] == eig.shape, (A.shape, eig.shape)
    d = eig.ndim - 1
    ncomp = A.shape[0]
    ce = wn.corner_sets(eig, d).transpose(0, 2, 1).reshape(-1, d + 1)
    cA = wn.corner_sets(np.moveaxis(A, 0, -1), d).transpose(0, 2, 1, 3).reshape(-1, d + 1, ncomp)
    o = np.argsort(ce, axis=1, kind="stable")
    w = 1.0 / (math.factorial(d) * float(np.prod(eig.shape[:d])))
    return np.take_along_axis(ce, o, 1), np.take_along_axis(cA, o[:, :, None], 1), w


def kappa(e, a):
    """e [S, d+1], a [S, d+1, ncomp] -> kappa_T [S, ncomp]"""
    d1 = e.shape[1]
    dev = e.sum(axis=1, keepdims=True) - d1 * e  # sum_l e_l - (d+1) e_i
    return factor(d1 - 1) * np.einsum("si,sic->sc", dev, a)


def correction_from(simplices, Es):
    """The correction term [nE, ncomp] from what sorted_simplices returned (share it among energy lists)."""
    e, a, w = simplices
    kap = kappa(e, a)
    lo, hi = e[:, 0], e[:, -1]
    Es = np.atleast_1d(np.asarray(Es, dtype=np.float64))
    out = np.zeros((len(Es), a.shape[2]))
    for i, E in enumerate(Es):
        inside = np.flatnonzero((lo <= E) & (E < hi))
        if len(inside):
            g = ln._g(e[inside], E)
            out[i] = np.array(_fs(g[:, None] * kap[inside])) * w
    return out


def correction(eig, A, Es):
    """w sum_T g_T(E) kappa_T at the energies Es: [nE, ncomp], to be added to wltm_numpy.wltm's N_A."""
    return correction_from(sorted_simplices(eig, A), Es)


def band_energy(eig, nstates, corrected=True, tol=1e-13):
    """(E_band, E_F) of a grid of eigenvalues: E_F by bisection on the plain N(E) = nstates of ltm_numpy, the band energy
    N_e(E_F) of wltm_numpy, plus the correction."""
    eig = np.asarray(eig, dtype=np.float64)
    lo, hi = float(eig.min()), float(eig.max())
    e = ln.kuhn_simplices(eig)
    w = 1.0 / (math.factorial(eig.ndim - 1) * float(np.prod(eig.shape[:-1])))
    slo, shi = e[:, 0], e[:, -1]

    def N(E):
        inside = (slo <= E) & (E < shi)
        return (math.fsum(ln._n(e[inside], E)) + np.count_nonzero(shi <= E)) * w

    while hi - lo > tol * max(1.0, abs(lo), abs(hi)):
        mid = 0.5 * (lo + hi)
        if N(mid) < nstates:
            lo = mid
        else:
            hi = mid
    E_F = hi
    Eb = wn.wltm(eig, eig, [E_F])[1][0, 0]
    if corrected:
        Eb += correction(eig, eig, [E_F])[0, 0]
    return Eb, E_F


def cosine_band(npt, d=3, t=(1.0, 1.0, 1.0), diag=0.0):
    """-2 sum_j t_j cos k_j + diag cos(k_1 + k_2) on the periodic grid k = 2 pi i / npt: [npt]*d + [1]"""
    k = 2.0 * np.pi * np.arange(npt) / npt
    ks = np.meshgrid(*([k] * d), indexing="ij")
    e = sum(-2.0 * t[j] * np.cos(ks[j]) for j in range(d))
    if diag and d >= 2:
        e = e + diag * np.cos(ks[0] + ks[1])
    return e[..., None]

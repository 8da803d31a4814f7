"""Orbital weights |U_ab(k)|^2 with LAPACK: what abz_rule_ltm_orbitals computes on the device, restated with numpy.

At a degenerate level numpy returns SOME orthonormal basis of the eigenspace, and so does the device; the two need not be
the same.  What both define is the sum of the weights over the level -- the diagonal of its spectral projector -- which
`cluster_sums` forms."""
import numpy as np


def weights(H):
    """H [nk, n, n] Hermitian (the upper triangle is read, as by Hermitian(h)) -> W [n(a), nk, n(b)] = |U_ab|^2, bands
    ascending: the layout of DeviceRule.ltm_elements."""
    H = np.asarray(H)
    if H.ndim == 1:  # scalar series
        return np.ones((1, len(H), 1))
    _, U = np.linalg.eigh(H, UPLO="U")
    return np.ascontiguousarray((np.abs(U) ** 2).transpose(1, 0, 2))


def clusters(e, tol):
    """Runs of ascending eigenvalues e [n] in which neighbours are closer than tol: a list of (first, one past last)."""
    e = np.asarray(e)
    out, a = [], 0
    for b in range(1, len(e) + 1):
        if b == len(e) or e[b] - e[b - 1] >= tol:
            out.append((a, b))
            a = b
    return out


def cluster_sums(e, W, tol):
    """e [nk, n] ascending, W [ncomp, nk, n] -> S [ncomp, nk, n]: every band carries the sum of W over the run of eigenvalues
    (neighbours closer than tol) it belongs to."""
    e, W = np.asarray(e), np.asarray(W)
    S = np.empty_like(W)
    for k in range(e.shape[0]):
        for a, b in clusters(e[k], tol):
            S[:, k, a:b] = W[:, k, a:b].sum(axis=1, keepdims=True)
    return S

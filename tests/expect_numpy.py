"""Band expectation values q_i = Re u_b^H Hermitian(O_i(k)) u_b with LAPACK: what abz_rule_ltm_expectation computes on the
device, restated with numpy on exported planes.

At a degenerate level numpy returns SOME orthonormal basis of the eigenspace, and so does the device; single expectations
then need not agree, their sums over the level (orbw_numpy.cluster_sums) do, and products of two are not defined."""
import numpy as np

from orbw_numpy import cluster_sums  # noqa: F401  (the level sums of the device tests)


def matrices(X):
    """Exported planes [nk, n, n], or [nk] of a scalar series, as [nk, n, n]."""
    X = np.asarray(X)
    return X.reshape(len(X), 1, 1) if X.ndim == 1 else X


def hermitian_upper(X):
    """Hermitian(X): the upper triangle and its conjugate, a real diagonal."""
    up = np.triu(X, 1)
    return up + np.conj(np.swapaxes(up, -1, -2)) + np.real(np.einsum("...ii->...i", X))[..., None] * np.eye(X.shape[-1])


def expectations(H, ops):
    """H [nk, n, n], ops: a list of [nk, n, n] -> q [nops, nk, n], bands ascending (eigh of the upper triangle of H)."""
    H = matrices(H)
    _, U = np.linalg.eigh(H, UPLO="U")
    return np.stack([np.einsum("kab,kac,kcb->kb", U.conj(), hermitian_upper(matrices(O)), U).real for O in ops])


def elements(H, ops, comps=None):
    """The element block [ncomp, nk, n] of the components `comps`: (i, -1) or i -> q_i, (i, j) -> q_i q_j; None: q in order."""
    q = expectations(H, ops)
    if comps is None:
        return q
    out = []
    for c in comps:
        i, j = (c, -1) if np.ndim(c) == 0 else c
        out.append(q[i] if j < 0 else q[i] * q[j])
    return np.stack(out)


def norms(ops):
    """max_k ||O_i(k)||_2 of every operator."""
    return [float(np.linalg.norm(hermitian_upper(matrices(O)), 2, axis=(1, 2)).max()) for O in ops]


def bounds(ops, comps=None, rel=1e-10):
    """rel max(1, max||O_i||) for a single, rel max(1, max||O_i|| max||O_j||) for a product, per component [ncomp]."""
    nrm = norms(ops)
    comps = list(range(len(ops))) if comps is None else comps
    out = []
    for c in comps:
        i, j = (c, -1) if np.ndim(c) == 0 else c
        out.append(rel * max(1.0, nrm[i] if j < 0 else nrm[i] * nrm[j]))
    return np.array(out)

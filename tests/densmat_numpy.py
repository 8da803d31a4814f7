"""numpy restatement of the density matrix of the tetrahedron method in the orbital basis (abz_rule_ltm_density_matrix):

    rho_pq(E) = sum_k sum_b w_b(k; E) U_pb(k) conj(U_qb(k))

with Bloechl's integration weights w_b(k; E) of tests/nodew_numpy.py and the band projectors of tests/gloc_ltm_numpy.py: one
einsum of the two.  `kind` is the kind of the weights: "states" (the occupation matrix), "corrected" (with the curvature
correction; those weights do go negative) or "dos" (the spectral-density matrix).

The upper triangle p <= q is kept and the lower one filled as its conjugate, with a real diagonal, as the library does: rho is
Hermitian to the bit."""
import numpy as np

import gloc_ltm_numpy as gl
import nodew_numpy as nw


def contract(W, P):
    """W [nE] + grid + [n] real, P [m, m] + grid + [n] complex -> rho [nE, m, m] = einsum(W, P); the upper triangle p <= q is
    kept and mirrored"""
    W, P = np.asarray(W, dtype=np.float64), np.asarray(P)
    assert P.shape[0] == P.shape[1] and P.shape[2:] == W.shape[1:], (P.shape, W.shape)
    m, nE, n = P.shape[0], W.shape[0], W.shape[-1]
    full = np.einsum("ekb,pqkb->epq", W.reshape(nE, -1, n), P.reshape(m, m, -1, n))
    up = np.triu(full, 1)
    return up + np.conj(np.swapaxes(up, 1, 2)) + np.einsum("epp->ep", full).real[:, :, None] * np.eye(m)


def density_matrix(eig, HP, Es, kind="states"):
    """rho [nE, m, m] of the eigenvalues eig [npt]*d + [n] and either H [npt]*d + [n, n] (m = n, the projectors come from
    numpy.linalg.eigh) or the projector tensor P [m, m] + [npt]*d + [n] itself (any m; only p <= q matters)."""
    eig = np.asarray(eig, dtype=np.float64)
    HP = np.asarray(HP)
    P = gl.projector_tensor(HP) if HP.ndim == eig.ndim + 1 else HP
    return contract(nw.node_weights(eig, Es, kind), P)

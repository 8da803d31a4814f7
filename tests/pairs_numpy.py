"""Band-pair energies and interband products with LAPACK: what abz_rule_ltm_pairs computes on the device, restated with numpy on
exported planes.  For the lower range [v0, v0 + nv) and the upper range [c0, c0 + nc) of the ascending bands, pseudo-band
p = (v - v0) nc + (c - c0):  Delta_p = e_c - e_v,  M^i_vc = u_v^H Hermitian(O_i) u_c,  component (i, j, part) = Re (0) or Im (1) of
M^i_vc conj(M^j_vc) -- a product no phase of u_v or u_c changes.

At a degenerate level numpy returns SOME orthonormal basis of the eigenspace, and so does the device: single pairs then need
not agree, the sums of a component over all pairs between two levels (level_pair_sums) do."""
import numpy as np

from expect_numpy import hermitian_upper, matrices, norms
from orbw_numpy import clusters


def pair_energies(eig, v0, nv, c0, nc):
    """eig [nk, n] -> [nk, nv nc], the subtraction the device makes."""
    return (eig[:, None, c0:c0 + nc] - eig[:, v0:v0 + nv, None]).reshape(len(eig), nv * nc)


def interband(H, ops, v0, nv, c0, nc, U=None):
    """M [nops, nk, nv, nc] complex from H [nk, n, n] (eigh of its upper triangle, or the given eigenvectors U) and ops [nk, n, n]."""
    if U is None:
        _, U = np.linalg.eigh(matrices(H), UPLO="U")
    Uv, Uc = U[:, :, v0:v0 + nv], U[:, :, c0:c0 + nc]
    return np.stack([np.einsum("kav,kab,kbc->kvc", Uv.conj(), hermitian_upper(matrices(O)), Uc) for O in ops])


def normalise(comps, nops):
    """Components as (i, j, part) triples: i -> (i, i, 0), (i, j) -> (i, j, 0), (i, j, "re" | "im" | 0 | 1); None: |M^i|^2 in order."""
    if comps is None:
        return [(i, i, 0) for i in range(nops)]
    out = []
    for c in comps:
        t = (c, c, 0) if np.ndim(c) == 0 else tuple(c)
        t = (t[0], t[1], 0) if len(t) == 2 else t
        out.append((int(t[0]), int(t[1]), {"re": 0, "im": 1}.get(t[2], t[2])))
    return out


def components(M, comps=None):
    """The element block [ncomp, nk, nv nc] from M [nops, nk, nv, nc]."""
    out = []
    for i, j, part in normalise(comps, len(M)):
        x = M[i] * np.conj(M[j])
        out.append((x.imag if part else x.real).reshape(M.shape[1], -1))
    return np.stack(out)


def elements(H, ops, v0, nv, c0, nc, comps=None):
    return components(interband(H, ops, v0, nv, c0, nc), comps)


def bounds(ops, comps=None, rel=1e-10):
    """rel max(1, max||O_i|| max||O_j||) per component [ncomp]: the bound of expect_numpy.bounds for a product."""
    nrm = norms(ops)
    return np.array([rel * max(1.0, nrm[i] * nrm[j]) for i, j, _ in normalise(comps, len(ops))])


def level_pair_sums(eig, A, v0, nv, c0, nc, tol):
    """A [ncomp, nk, nv nc] summed over the pairs between two levels: every pair (v, c) of a node gets the sum over the pairs
    (v', c') with v' in the level of v and c' in the level of c (levels: orbw_numpy.clusters of the node's eigenvalues)."""
    A = np.asarray(A).reshape(A.shape[0], A.shape[1], nv, nc)
    S = np.empty_like(A)
    for k in range(A.shape[1]):
        cl = clusters(eig[k], tol)
        level = np.empty(len(eig[k]), dtype=int)
        for m, (a, b) in enumerate(cl):
            level[a:b] = m
        lv, lc = level[v0:v0 + nv], level[c0:c0 + nc]
        same_v = (lv[:, None] == lv[None, :]).astype(float)  # [v, v']
        same_c = (lc[:, None] == lc[None, :]).astype(float)
        S[:, k] = np.einsum("vw,awd,cd->avc", same_v, A[:, k], same_c)
    return S.reshape(A.shape[0], A.shape[1], nv * nc)

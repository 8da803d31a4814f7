"""numpy restatement of the integration weights of the optimized tetrahedron method (helper of
test_ltm_node_weights_optimized_cpu.py / test_gpu_ltm_node_weights_optimized.py, not a conftest).

The scatter form of optltm_numpy.py.  For every path (permutation of the axes) and cell the band is taken at the 20 stencil
points (`stencil_values`), the effective corner energies are e' = P e with the projection derived in exact rationals
(`projection_float`), the corners are sorted (stable), `_weights` gives the corner weights of the linear rule inside the
window e'_1 <= E < e'_4, a simplex with max e' <= E gives 1/4 to each corner (states) and nothing to the DOS, and the weights
are brought back to path order.  An element takes the same projection, so sum_m w'_m A'_m = sum_j (P^T w')_j A(p_j): the
point weights P^T w' are added at cell + off_j with np.roll, every index mod npt, and the sum is multiplied by the simplex
weight 1 / (6 npt^3).  Nothing here reads a table of the kernels; it works for any float type.
"""
import itertools

import numpy as np

import optltm_numpy as on


def corner_weights(e, Es, states):
    """Effective corner energies e [K, 4] in path order -> [nE, K, 4]: the corner weights of the linear rule in path order,
    unit = one simplex."""
    o = np.argsort(e, axis=1, kind="stable")
    es = np.take_along_axis(e, o, 1)
    lo, hi = es[:, 0], es[:, -1]
    out = np.zeros((len(Es),) + e.shape, dtype=e.dtype)
    for i, E in enumerate(Es):
        ws = np.zeros_like(es)
        inside = (lo <= E) & (E < hi)
        if inside.any():
            ws[inside] = on._weights(es[inside], E, states)
        if states:
            ws[hi <= E] = e.dtype.type(1) / e.dtype.type(4)
        np.put_along_axis(out[i], o, ws, 1)  # sorted corner s is corner o[s] of the path
    return out


def node_weights(eig, Es, states, dtype=np.float64):
    """eig [npt, npt, npt, n] ascending eigenvalues, energies Es -> w_b(k; E) as [nE, npt, npt, npt, n] in `dtype`."""
    eig = np.asarray(eig, dtype=dtype)
    npt, n = eig.shape[0], eig.shape[-1]
    assert eig.shape[:3] == (npt, npt, npt)
    Es = np.atleast_1d(np.asarray(Es, dtype=dtype))
    P = on.projection_float(dtype)
    W = np.zeros((len(Es),) + eig.shape, dtype=dtype)
    for perm in itertools.permutations(range(3)):
        x = on.stencil_values(eig, perm)                      # [20, ncell, n]
        ep = np.tensordot(P, x, axes=(1, 0))                  # [4, ncell, n]
        cw = corner_weights(np.moveaxis(ep, 0, -1).reshape(-1, 4), Es, states)  # [nE, ncell n, 4]
        pw = np.matmul(cw, P)                                 # [nE, ncell n, 20]: P^T w'
        for j, off in enumerate(on.points(perm)):
            g = pw[..., j].reshape(W.shape)                   # at the cell
            for ax in range(3):
                if off[ax]:
                    g = np.roll(g, int(off[ax]), axis=ax + 1)  # to the point cell + off, wrapped
            W += g
    return W * (dtype(1) / dtype(6 * npt ** 3))

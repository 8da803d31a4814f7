"""numpy restatement of Bloechl's integration weights per grid point and band (helper of test_ltm_node_weights_cpu.py /
test_gpu_ltm_node_weights.py, not a conftest).

w_b(k; E) with  N_A(E) = sum_k sum_b w_b(k; E) A_b(k)  for any A (and g_A, and the curvature correction of N_A), on the mesh of
ltm_numpy.py.  A GEOMETRIC restatement that shares nothing with the closed forms of kernels_ltm_nodew.hip: it is the scatter
form of wltm_numpy.py.  The corners of every simplex are wltm_numpy.corner_sets of the array of flat (k, b) indices; the pieces
that fill {e < E} and the cut {e = E} are wltm_numpy._pieces, matrices B of barycentric coordinates with one row per vertex.

* States: a sub-simplex B holds |det B| of its parent's volume, and the integral of the barycentric coordinate lambda_i over it
  is that volume times the mean of lambda_i over B's vertices, so corner i gets  sum_B |det B| B.mean(axis=0)[i];  where the
  pieces fill the part ABOVE E, 1 / (d+1) minus that.  A simplex wholly below E gives 1 / (d+1) to each corner.
* DOS: the cone-over-the-cut densities of wltm_numpy (apex = the corner farthest from E) times C.mean(axis=0).
* Correction: g_T(E) f_d (sum_l e_l - (d+1) e_i) to corner i of a simplex with e_1 <= E < e_{d+1}: ltm_numpy._g,
  bloechl_numpy.factor.

The shares are scattered onto the (k, b) they belong to with np.add.at (at most (d+1)! terms per entry) and multiplied by the
simplex weight 1 / (d! nk).  Half-open regions e_i <= E < e_{i+1} as everywhere; a flat simplex gives nothing to the DOS.
"""
import math

import numpy as np

import bloechl_numpy as bn
import ltm_numpy as ln
import wltm_numpy as wn

KINDS = ("dos", "states", "corrected")


def simplices(eig):
    """eig [npt]*d + [n] -> (e [S, d+1] ascending, idx [S, d+1] the flat (k, b) index of each sorted corner, d)."""
    eig = np.asarray(eig, dtype=np.float64)
    d = eig.ndim - 1
    flat = np.arange(eig.size).reshape(eig.shape)
    ce = wn.corner_sets(eig, d).transpose(0, 2, 1).reshape(-1, d + 1)
    ci = wn.corner_sets(flat, d).transpose(0, 2, 1).reshape(-1, d + 1)
    o = np.argsort(ce, axis=1, kind="stable")
    return np.take_along_axis(ce, o, 1), np.take_along_axis(ci, o, 1), d


def shares(e, E, kind, d):
    """Sorted corner energies e [K, d+1] of simplices with e_1 <= E < e_{d+1} -> what each corner gets, [K, d+1], unit = one
    simplex."""
    d1 = d + 1
    out = np.zeros(e.shape)
    m_all = np.count_nonzero(e <= E, axis=1)
    for m in range(1, d1):
        sel = np.flatnonzero(m_all == m)
        if not len(sel):
            continue
        es = e[sel]
        below, complement, cut = wn._pieces(es, E)
        if kind == "dos":
            apex = np.where((E - es[:, 0]) >= (es[:, -1] - E), 0, d)
            e_apex = np.take_along_axis(es, apex[:, None], 1)[:, 0]
            tip = np.eye(d1)[apex][:, None, :]
            out[sel] = sum((d * np.abs(np.linalg.det(np.concatenate([C, tip], axis=1))) / np.abs(e_apex - E))[:, None] * C.mean(axis=1)
                           for C in cut)
            continue
        part = sum(np.abs(np.linalg.det(B))[:, None] * B.mean(axis=1) for B in below)
        if complement:
            part = 1.0 / d1 - part
        if kind == "corrected":
            part = part + ln._g(es, E)[:, None] * bn.factor(d) * (es.sum(axis=1, keepdims=True) - d1 * es)
        out[sel] = part
    return out


def node_weights_from(simp, shape, Es, kind="states"):
    """The weights [nE] + shape from what simplices() returned (share it among energy lists and kinds)."""
    assert kind in KINDS, kind
    e, idx, d = simp
    nk = int(np.prod(shape[:d]))
    w = 1.0 / (math.factorial(d) * float(nk))
    lo, hi = e[:, 0], e[:, -1]
    Es = np.atleast_1d(np.asarray(Es, dtype=np.float64))
    W = np.zeros((len(Es), int(np.prod(shape))))
    for i, E in enumerate(Es):
        if kind != "dos":
            full = np.flatnonzero(hi <= E)
            np.add.at(W[i], idx[full].reshape(-1), 1.0 / (d + 1))
        inside = np.flatnonzero((lo <= E) & (E < hi))
        if len(inside):
            np.add.at(W[i], idx[inside].reshape(-1), shares(e[inside], E, kind, d).reshape(-1))
    return (W * w).reshape((len(Es),) + tuple(shape))


def node_weights(eig, Es, kind="states"):
    """eig [npt]*d + [n] ascending eigenvalues, energies Es -> w_b(k; E) as [nE] + eig.shape; kind: "dos", "states" or
    "corrected" (states with the curvature correction)."""
    eig = np.asarray(eig, dtype=np.float64)
    return node_weights_from(simplices(eig), eig.shape, Es, kind)

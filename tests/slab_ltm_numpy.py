"""numpy restatement of the tetrahedron sums of a SLAB of the grid (helper of test_ltm_slab_cpu.py /
test_gpu_ltm_slab.py, not a conftest).

In the [npt]*d + [n] array of ltm_numpy.rule_eigenvalues axis 0 is the outermost variable (C-order reshape of the export,
i_1 fastest), so the slab [z0, z1) of abz_ptr_rule_build_slab is rows z0 .. z1-1 of it.  A slab's partial sum runs over the
cells whose outermost index lies in [z0, z1): their corners reach one plane further, plane z1 mod npt -- the halo plane of
abz_rule_ltm_halo.  Every simplex keeps the whole grid's weight 1 / (d! npt^d), so the partial sums of a partition of
[0, npt) add up to the whole grid's value.

Only the enumeration of the cells is new here.  The simplices are evaluated by the per-simplex code of the whole-grid
restatements: ltm_numpy._g / _n, wltm_numpy._pieces with the arithmetic of wltm_numpy.wltm's driver around it (volume x
mean of the vertex values; cone over the cut), bloechl_numpy.kappa; sums over simplices as there (math.fsum; blocks of 16
through math.fsum for the weighted sums).
"""
import itertools
import math

import numpy as np

import bloechl_numpy as bn
import ltm_numpy as ln
import wltm_numpy as wn


def extend(arr, z0, z1):
    """Rows [z0, z1) of the whole-grid array `arr` ([npt]*d + [...]) followed by the halo plane z1 mod npt."""
    npt = arr.shape[0]
    assert 0 <= z0 < z1 <= npt
    h = z1 % npt
    return np.concatenate([arr[z0:z1], arr[h:h + 1]], axis=0)


def corner_sets(ext, d):
    """wltm_numpy.corner_sets for the cells of the first nz = len(ext) - 1 planes of an extended slab: [nsimplex, d + 1, ...].
    The outermost index (axis 0) does not wrap -- the roll's wrap-around only reaches the cells of the halo plane, which are
    dropped -- the other axes wrap mod npt as on the whole grid."""
    nz = ext.shape[0] - 1
    out = []
    for perm in itertools.permutations(range(d)):
        cs = [ext]
        cur = ext
        for ax in perm:
            cur = np.roll(cur, -1, axis=ax)
            cs.append(cur)
        out.append(np.stack([c[:nz].reshape((-1,) + ext.shape[d:]) for c in cs], axis=1))
    return np.concatenate(out, axis=0)


def _weight(ext):
    d = ext.ndim - 1  # (>= 2: a slab needs a variable beside the outermost one, and that axis has the grid's npt)
    return 1.0 / (math.factorial(d) * float(ext.shape[1]) ** d)


def ltm(ext, Es):
    """(g, N) partial sums of the slab whose extended eigenvalues are `ext` [nz + 1] + [npt]*(d-1) + [n]: the arithmetic of
    ltm_numpy.ltm on the slab's simplices."""
    ext = np.asarray(ext, dtype=np.float64)
    d = ext.ndim - 1
    e = np.sort(corner_sets(ext, d).transpose(0, 2, 1).reshape(-1, d + 1), axis=1)
    lo, hi = e[:, 0], e[:, -1]
    weight = _weight(ext)
    Es = np.atleast_1d(np.asarray(Es, dtype=np.float64))
    g = np.zeros(len(Es))
    N = np.zeros(len(Es))
    for i, E in enumerate(Es):
        inside = (lo <= E) & (E < hi)
        below = np.count_nonzero(hi <= E)
        ei = e[inside]
        if len(ei):
            g[i] = math.fsum(ln._g(ei, E)) * weight
            N[i] = (math.fsum(ln._n(ei, E)) + below) * weight
        else:
            N[i] = below * weight
    return g, N


def sorted_simplices(ext, Aext):
    """bloechl_numpy.sorted_simplices for a slab: (e [S, d+1] ascending, a [S, d+1, ncomp] carried along, weight)."""
    ext = np.asarray(ext, dtype=np.float64)
    Aext = np.asarray(Aext, dtype=np.float64)
    if Aext.shape == ext.shape:
        Aext = Aext[None]
    assert Aext.shape[1:] == ext.shape, (Aext.shape, ext.shape)
    d = ext.ndim - 1
    ncomp = Aext.shape[0]
    ce = corner_sets(ext, d).transpose(0, 2, 1).reshape(-1, d + 1)
    cA = corner_sets(np.moveaxis(Aext, 0, -1), d).transpose(0, 2, 1, 3).reshape(-1, d + 1, ncomp)
    o = np.argsort(ce, axis=1, kind="stable")
    return np.take_along_axis(ce, o, 1), np.take_along_axis(cA, o[:, :, None], 1), _weight(ext)


def wltm_from(simplices, Es):
    """(g_A, N_A) [nE, ncomp] partial sums of a slab from what sorted_simplices returned: wltm_numpy.wltm's driver (sub-simplices
    below E and the cut from wltm_numpy._pieces; volume x mean of the vertex values, cone over the cut)."""
    ce, cA, w = simplices
    d1 = ce.shape[1]
    d = d1 - 1
    ncomp = cA.shape[2]
    lo, hi = ce[:, 0], ce[:, -1]
    means = cA.mean(axis=1)
    Es = np.atleast_1d(np.asarray(Es, dtype=np.float64))
    g = np.zeros((len(Es), ncomp))
    N = np.zeros((len(Es), ncomp))
    for i, E in enumerate(Es):
        Nc = [[v] for v in bn._fs(means[hi <= E])] if np.any(hi <= E) else [[] for _ in range(ncomp)]
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
                below, complement, cut = wn._pieces(e, E)
                vmean = lambda B: np.einsum("kv,kvc->kc", B.mean(axis=1), a)
                part = sum(np.abs(np.linalg.det(B))[:, None] * vmean(B) for B in below)
                if complement:
                    part = a.mean(axis=1) - part
                apex = np.where((E - e[:, 0]) >= (e[:, -1] - E), 0, d)
                e_apex = np.take_along_axis(e, apex[:, None], 1)[:, 0]
                tip = np.eye(d1)[apex][:, None, :]
                dens = sum((d * np.abs(np.linalg.det(np.concatenate([Cm, tip], axis=1))) / np.abs(e_apex - E))[:, None] *
                           vmean(Cm) for Cm in cut)
                for c, col in enumerate(bn._fs(part)):
                    Nc[c].append(col)
                for c, col in enumerate(bn._fs(dens)):
                    gc[c].append(col)
        for c in range(ncomp):
            N[i, c] = math.fsum(Nc[c]) * w
            g[i, c] = math.fsum(gc[c]) * w
    return g, N


def wltm(ext, Aext, Es):
    return wltm_from(sorted_simplices(ext, Aext), Es)


def correction(ext, Aext, Es):
    """The slab's share of Bloechl's correction, w sum_T g_T(E) kappa_T over the slab's simplices (bloechl_numpy.correction_from
    takes any list of sorted simplices)."""
    return bn.correction_from(sorted_simplices(ext, Aext), Es)


def slabs(npt, world):
    """[(z0, z1)] of the ranks of a k-sharded grid (series.slab_range), empty ones included."""
    return [((npt * r) // world, (npt * (r + 1)) // world) for r in range(world)]

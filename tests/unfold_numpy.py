"""numpy side of the eigenvalue unfolding (helper of test_ltm_unfold_cpu.py / test_gpu_ltm_unfold.py, not a conftest).

A symmetry S of the zone is an integer matrix on the grid indices mod npt; eigenvalues are invariant, e_b(S k) = e_b(k),
so the eigenvalues of the whole grid are those of one node per orbit, gathered through the orbit map.  Flat grid
indices have i_1 fastest (the node order of a full-grid rule's export)."""
import itertools

import numpy as np


def grid_points(npt, d):
    """[npt^d, d] grid indices, flat index i_1 fastest."""
    flat = np.arange(npt ** d, dtype=np.int64)
    return np.stack([(flat // npt ** j) % npt for j in range(d)], axis=1)


def flat_index(idx, npt):
    idx = np.asarray(idx, dtype=np.int64)
    return sum(idx[:, j] * npt ** j for j in range(idx.shape[1]))


def _int_syms(syms, d):
    S = np.rint(np.asarray(syms, dtype=np.float64)).astype(np.int64).reshape(-1, d, d)
    assert np.allclose(S, np.asarray(syms, dtype=np.float64).reshape(-1, d, d))
    return S


def images(npt, d, syms):
    """[nsyms, npt^d] flat index of the image of every grid point under every symmetry."""
    v = grid_points(npt, d)
    return np.stack([flat_index((v @ S.T) % npt, npt) for S in _int_syms(syms, d)])


def irreducible(npt, d, syms):
    """(idx [nirr, d], w [nirr]): the smallest image of every orbit in flat order, and the number of distinct images of
    it -- what symptr_rule returns."""
    img = images(npt, d, syms)
    flat = np.arange(npt ** d)
    rep = np.all(img >= flat[None], axis=0)
    w = np.array([len(set(img[:, k])) for k in flat[rep]], dtype=np.int64)
    return grid_points(npt, d)[rep].astype(np.int32), w


def orbit_map(npt, d, syms, x):
    """node_of [npt^d]: for every grid point the node of the list `x` [nk, d] (fractional coordinates, as a rule exports
    them) that is the point itself or one of its images.  Raises if a point has none."""
    idx = np.rint(np.asarray(x, dtype=np.float64).reshape(-1, d) * npt).astype(np.int64) % npt
    rank = np.full(npt ** d, -1, dtype=np.int64)
    rank[flat_index(idx, npt)] = np.arange(len(idx))
    node_of = rank.copy()
    for row in images(npt, d, syms):
        todo = node_of < 0
        node_of[todo] = rank[row[todo]]
    if np.any(node_of < 0):
        raise ValueError(f"{np.count_nonzero(node_of < 0)} grid points have no node in their orbit")
    return node_of


def unfold(eig_nodes, node_of, npt, d):
    """eigenvalues of the nodes [nk, n] -> [npt]*d + [n], the shape ltm_numpy.rule_eigenvalues gives."""
    e = np.asarray(eig_nodes)[node_of]
    return e.reshape((npt,) * d + (e.shape[-1],))


def grid_flat(eig_grid):
    """[npt]*d + [n] indexed [i_1, ..., i_d] (ltm_numpy.grid_eigenvalues) -> [npt^d, n] with i_1 fastest."""
    d = eig_grid.ndim - 1
    return np.ascontiguousarray(eig_grid.transpose(tuple(range(d - 1, -1, -1)) + (d,))).reshape(-1, eig_grid.shape[-1])


def symmetrise_coefficients(c, first):
    """c [M, M, M, n, n] with frequencies first .. -first on every axis -> its average over the 48 signed permutations of
    the three lattice axes (transposes and flips of the coefficient axes)."""
    c = np.asarray(c)
    assert c.ndim == 5 and len(set(c.shape[:3])) == 1 and all(int(f) == -(c.shape[0] // 2) for f in first)
    acc = np.zeros_like(c)
    count = 0
    for perm in itertools.permutations(range(3)):
        cp = c.transpose(perm + (3, 4))
        for flips in itertools.product((False, True), repeat=3):
            axes = tuple(j for j in range(3) if flips[j])
            acc += np.flip(cp, axes) if axes else cp
            count += 1
    assert count == 48
    return acc / 48.0


def symmetrise(series):
    """The oracle FourierSeries with its coefficient array averaged over the 48 signed permutations of the three lattice
    axes, whose frequency ranges are symmetric about 0.  The average is Hermitian per R like the input, and
    H(S k) = H(k) for every cubic operation S."""
    import abz_oracle as orc
    assert series.d == 3
    return orc.FourierSeries(symmetrise_coefficients(series.c, series.first), period=1.0, first=series.first, ndim=3)

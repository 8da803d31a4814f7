"""numpy restatement of the IAI building blocks (helper of test_iai_blocks_cpu.py / test_gpu_iai_blocks.py, not a conftest).

The C ABI exports three entry points for a caller that keeps its own adaptive loop (include/abzhip.h, "IAI building blocks"):
abz_contract_nodes, abz_eval_line_nodes, abz_release_level; `DeviceSeries` mirrors them.  This module states the same three
operations on the oracle's series (abz_oracle.contract / abz_oracle.phases), every built-in integrand at a list of nodes,
and the host-driven loop the entry points exist for: a depth-first nested GK(7,15) integration in the shape of
abz_oracle.nested_quad whose every node batch is one call of a building block.

* a slot is the position of a contracted series in its level's list; every contract_nodes call appends, so slots are
  numbered consecutively per level from the level's current count;
* level d holds the series itself as its only slot 0;
* release_level(level) empties the lists of the levels below `level`;
* a parent that is not a live slot raises ValueError (the ABI answers ABZ_ERR_ARG).
"""
import numpy as np

import abz_oracle as orc

F_ONE, F_LINEAR, F_LINEAR_X, F_DOS, F_TRGLOC, F_GLOC, F_DOS_EIG = range(7)  # include/abzhip.h


def ncomp(fid, n, d):
    return {F_GLOC: n * n, F_LINEAR_X: d}.get(fid, 1)


def integrand_ref(fid, n, d, params, sweep, X, H):
    """Built-in integrand `fid` at N nodes: X [N, d] coordinates (x_1 first), H [N, n, n] series values -> complex
    [N, ncomp].  F_GLOC comes column-major (element (a, b) at a + n b), the order the ABI documents."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, d)
    H = np.asarray(H, dtype=np.complex128).reshape(len(X), n, n)
    if fid == F_ONE:
        v = orc.f_one()(X, H)[:, None]
    elif fid == F_LINEAR:
        v = orc.f_linear(params[0], params[1])(X, H[:, 0, 0])[:, None]
    elif fid == F_LINEAR_X:
        v = orc.f_linear_x(params[0], params[1])(X, H[:, 0, 0])
    elif fid == F_DOS:
        v = orc.f_dos(params[0], sweep)(X, H)[:, None]
    elif fid == F_TRGLOC:
        v = np.trace(orc.f_gloc(params[0], sweep)(X, H), axis1=-2, axis2=-1)[:, None]
    elif fid == F_GLOC:
        v = np.transpose(orc.f_gloc(params[0], sweep)(X, H), (0, 2, 1)).reshape(len(X), n * n)
    elif fid == F_DOS_EIG:  # (eta / pi) sum_b 1 / ((w - e_b)^2 + eta^2), e = eigenvalues of Hermitian(H): the upper triangle
        e = np.linalg.eigvalsh(H, UPLO="U")
        v = ((params[0] / np.pi) / ((sweep - e) ** 2 + params[0] ** 2)).sum(axis=1)[:, None]
    else:
        raise ValueError(f"unknown integrand id {fid}")
    return np.asarray(v, dtype=np.complex128)


class NumpyBlocks:
    """The three building blocks on an oracle series `so` (abz_oracle.FourierSeries)."""

    def __init__(self, so):
        self.so = so
        self.d = so.d
        self.sets = {L: [] for L in range(1, so.d)}  # level -> contracted series, indexed by slot
        self.sets[so.d] = [so]

    def _parent(self, who, level, p, i):
        live = len(self.sets[level])
        if not 0 <= p < live:
            raise ValueError(f"{who}: parents[{i}] = {p} is not a live level-{level} slot ({live} live slots)")
        return self.sets[level][p]

    def contract_nodes(self, src_level, parents, x):
        if not 2 <= src_level <= self.d:
            raise ValueError(f"src_level = {src_level} must be in 2..d")
        parents = np.asarray(parents, dtype=np.int64).reshape(-1)
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        assert len(parents) == len(x)
        new = [orc.contract(self._parent("contract_nodes", src_level, int(p), i), xi) for i, (p, xi) in enumerate(zip(parents, x))]
        dst = self.sets[src_level - 1]
        base = len(dst)
        dst.extend(new)  # (nothing is appended when a parent was refused)
        return np.arange(base, base + len(new), dtype=np.int64)

    def eval_line_nodes(self, parents, x, integrand, params, sweep, tail=None):
        d, n = self.d, self.so.n
        parents = np.asarray(parents, dtype=np.int64).reshape(-1)
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        assert len(parents) == len(x)
        if integrand in (F_LINEAR, F_LINEAR_X) and n != 1:
            raise ValueError("F_LINEAR(_X) needs a scalar (n = 1) series")
        if integrand == F_LINEAR_X and d > 1 and tail is None:
            raise ValueError("F_LINEAR_X needs the outer coordinates (tail)")
        for i, p in enumerate(parents):
            self._parent("eval_line_nodes", 1, int(p), i)
        X = np.zeros((len(x), d))
        X[:, 0] = x
        if tail is not None and d > 1:
            X[:, 1:] = np.asarray(tail, dtype=np.float64).reshape(len(x), d - 1)
        out = np.empty((len(x), ncomp(integrand, n, d)), dtype=np.complex128)
        # the nodes of one line in one batch, in their order: the innermost step of abz_oracle.nested_quad, operation for operation
        for p in dict.fromkeys(int(p) for p in parents):
            sel = np.flatnonzero(parents == p)
            cur = self.sets[1][p]
            ph = orc.phases(cur, 0, x[sel])  # (N, M)
            vs = np.tensordot(ph, cur.c, axes=(1, 0))  # (N, n, n)
            out[sel] = integrand_ref(integrand, n, d, params, sweep, X[sel], vs)
        return out

    def release_level(self, level):
        if not 1 <= level <= self.d:
            raise ValueError("release_level: bad level")
        for L in range(1, level):
            self.sets[L].clear()


def nested_gk(blocks, d, lims, fid, params, sweep, abstol=None, reltol=None):
    """Depth-first nested GK(7,15) in the shape of abz_oracle.nested_quad, driven through the building blocks `blocks`
    (NumpyBlocks or DeviceSeries): every batch g(xs) of an outer variable is ONE contract_nodes call whose nodes share one
    parent, every batch of the innermost variable ONE eval_line_nodes call, and once the children of an outer batch are
    consumed the levels below are released.  Returns (I [ncomp] complex, E, numevals)."""
    count = [0]
    last_err = [0.0]

    def level(L, parent, lims_l, tail, atol_l):
        segs = tuple(lims_l.segs())
        if L == 1:
            def g(xs):
                count[0] += len(xs)
                T = np.tile(np.asarray(tail, dtype=np.float64), (len(xs), 1)) if tail else None
                return blocks.eval_line_nodes(np.full(len(xs), parent, dtype=np.int64), xs, fid, params, sweep, tail=T)
        else:
            def g(xs):
                slots = blocks.contract_nodes(L, np.full(len(xs), parent, dtype=np.int64), xs)
                out = []
                for x, slot in zip(xs, slots):
                    inner = lims_l.fix(x)
                    isegs = inner.segs()
                    ln = isegs[-1] - isegs[0]
                    at = None if atol_l is None else atol_l / ln
                    out.append(level(L - 1, int(slot), inner, (x,) + tail, at))
                blocks.release_level(L)
                return out
        I, E, _ = orc.auxquadgk(g, segs, atol=atol_l, rtol=reltol)
        last_err[0] = E
        return I

    u = level(d, 0, lims, (), abstol)
    return u, last_err[0], count[0]

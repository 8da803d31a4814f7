"""Fourier series container + its device-resident twin and cached PTR rules.

Mirrors FourierSeries / FourierWorkspace as the reference uses them (FourierSeriesEvaluators v1
semantics, ref docs/src/examples.md:26-42, src/fourier.jl:56-86): all arithmetic happens in
libabzhip.so on the GPU.
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import _lib as L


class FourierSeries:
    """s(x) = sum_i c[i] exp(2 pi i sum_j (i_j + o_j) x_j / t_j), i_j 1-based like Julia.

    `c`: array of shape (M_1..M_d) (scalar series) or (M_1..M_d, n, n) (matrix valued);
    `period`: scalar or d-tuple; `offset`: FourierSeriesEvaluators' offset (index shift), or give
    `first` = the integer frequency of c[0] along each dim (an OffsetArray's first axis value).
    ref: test/dos.jl:114 (`period=, offset=`), test/utils.jl:3-9, aps_example/aps_example.jl:15-27.
    """

    def __init__(self, c, period=1.0, offset=0, *, first=None, ndim=None):
        c = np.asarray(c)
        if ndim is None:
            ndim = c.ndim - 2 if (c.ndim >= 3 and c.shape[-1] == c.shape[-2]) else c.ndim
        self.d = int(ndim)
        if not 1 <= self.d <= 3:
            raise ValueError("FourierSeries: 1 <= ndim <= 3 supported")
        self.scalar = c.ndim == self.d
        if self.scalar:
            c = c.reshape(c.shape + (1, 1))
        if c.ndim != self.d + 2 or c.shape[-1] != c.shape[-2]:
            raise ValueError("coefficient array must be (M_1..M_d) or (M_1..M_d, n, n)")
        self.c = np.array(c, dtype=np.complex128)
        self.n = int(c.shape[-1])
        self.t = tuple(float(p) for p in (period if np.ndim(period) else (period,) * self.d))
        if first is not None:
            self.first = tuple(int(v) for v in (first if np.ndim(first) else (first,) * self.d))
        else:
            off = offset if np.ndim(offset) else (offset,) * self.d
            self.first = tuple(int(o) + 1 for o in off)
        self._dev = {}

    # fields named like the reference (test/dos.jl:122,129)
    @property
    def o(self):
        return tuple(f - 1 for f in self.first)

    @property
    def dims(self):
        return self.c.shape[: self.d]

    def invalidate(self):
        """Call after mutating `c` in place (ref: DOSCache.isfresh, test/dos.jl:123-124): every device copy
        gets the new coefficients and its cached rules are re-evaluated before their next use.  Handles held
        elsewhere (a solver's cacheval, a second DOSCache on the same series) stay valid."""
        self._dev = {k: dev for k, dev in self._dev.items() if dev._h is not None}
        for dev in self._dev.values():
            dev.update()

    def device(self, ctx=None, pivoting=None):
        """The series' copy on the device of `ctx`.  pivoting "none" / "partial": set that mode on it
        (DeviceSeries.set_pivoting); None leaves the copy's mode alone."""
        ctx = ctx or L.Context.default()
        dev = self._dev.get(id(ctx))
        if dev is None:
            dev = DeviceSeries(self, ctx)
            self._dev[id(ctx)] = dev
        if pivoting is not None:
            dev.set_pivoting(pivoting)
        return dev

    def derivative(self, j):
        """The series of d s / d(x_j / t_j): same dims, `first` and period, every coefficient times 2 pi i (i_j + o_j) -- the
        derivative with respect to the fractional coordinate, the convention of a rule's velocity planes
        (v_j = <dH/dx_j> t_j); divide by t_j for d/dx_j.  A Hermitian series has a Hermitian derivative."""
        j = int(j)
        if not 0 <= j < self.d:
            raise ValueError(f"FourierSeries.derivative: variable {j} outside 0..{self.d - 1}")
        shape = [1] * (self.d + 2)
        shape[j] = -1
        fac = 2j * np.pi * (self.first[j] + np.arange(self.c.shape[j], dtype=np.float64))
        out = FourierSeries(self.c * fac.reshape(shape), period=self.t, first=self.first, ndim=self.d)
        out.scalar = self.scalar
        return out

    def __call__(self, x):
        """Evaluate at one point (the fallback evaluator, ref src/fourier.jl:120-122)."""
        v = self.device().eval_nodes(np.atleast_2d(np.asarray(x, dtype=np.float64)))[0]
        return v


def julia_coefficient_order(c, d):
    """(M_1..M_d, n, n) numpy array -> flat complex array in the reference's memory order
    (block column-major, i_1 fastest ... i_d slowest)."""
    axes = tuple(range(d - 1, -1, -1)) + (d + 1, d)
    return np.ascontiguousarray(np.transpose(c, axes)).reshape(-1)


PIVOTING_MODES = {"none": L.PIVOT_NONE, "partial": L.PIVOT_PARTIAL}


class DeviceSeries:
    """abz_series handle + cache of device-resident rules keyed by (npt, symmetry set, want)."""

    def __init__(self, s: FourierSeries, ctx):
        self.s = s
        self.ctx = ctx
        flat = julia_coefficient_order(s.c, s.d)
        buf = np.ascontiguousarray(flat.view(np.float64))
        _, pbuf = L.f64(buf)
        dims, pdims = L.i32(np.array(s.dims, dtype=np.int32))
        first, pfirst = L.i32(np.array(s.first, dtype=np.int32))
        per, pper = L.f64(np.array(s.t))
        h = C.c_void_p()
        L.check(L.lib().abz_series_create(ctx.h, pbuf, s.d, pdims, pfirst, pper, s.n, C.byref(h)))
        self.h = h
        self.rules = {}
        self.kshard = None     # (rank, world): rules hold this rank's share of the nodes (dist.kshard)
        self.allreduce = None  # callable summing a float64 array over the ranks of the shard group
        self.rule_bytes = 0
        self.max_rule_bytes = 96 << 30  # keep rules resident in the 288 GB of HBM, LRU beyond this
        self.generation = 0  # bumped by update(): rules evaluated from older coefficients refill before use
        # the finalizer holds the raw handle only: passing `self.rules` kept every dropped series alive for ever
        # (registry -> rules -> rule.dev -> this object); the library reference-counts series <- rule, so the rules'
        # own finalizers may run before or after this one
        self._fin = weakref.finalize(self, DeviceSeries._destroy, h)

    @staticmethod
    def _destroy(h):
        try:
            if h:
                L.lib().abz_series_destroy(h)
        except Exception:
            pass

    def close(self):
        for r in list(self.rules.values()):
            r.close()
        self.rules.clear()
        self.rule_bytes = 0
        self._fin()
        self._h = None

    @property
    def h(self):
        if self._h is None:
            raise L.AbzError("DeviceSeries was closed")
        return self._h

    @h.setter
    def h(self, v):
        self._h = v

    def update(self, c=None):
        """Upload new coefficients of the same shape.  Every cached rule is stale from here on and is
        re-evaluated in place (abz_rule_rebuild, which also refreshes its Hermitian flag) before its next
        use -- the reference rebuilds its rule from the current series on every solve.  New coefficients
        `c` replace the host series' array and go to EVERY live device copy of the series (one per context
        it was used on): a copy left behind would integrate the old coefficients."""
        if c is not None:
            c = np.asarray(c, dtype=np.complex128)
            if c.shape != self.s.c.shape:
                c = c.reshape(self.s.c.shape)
            self.s.c = np.array(c)
            for dev in list(self.s._dev.values()):
                if dev is not self and dev._h is not None:
                    dev._upload()
        self._upload()

    def _upload(self):
        buf = np.ascontiguousarray(julia_coefficient_order(self.s.c, self.s.d).view(np.float64))
        L.check(L.lib().abz_series_update(self.h, buf.ctypes.data_as(L.c_f64p)))
        self.generation += 1
        if any(r.want & L.WANT_H_COMPACT for r in self.rules.values()) and not self.hermitian():
            self.drop_rules()  # upper-triangle rules cannot hold the values of a series that stopped being Hermitian

    # ---- how the resolvent integrands invert (abz_series_set_pivoting)
    def set_pivoting(self, mode):
        """"none": the default routes.  "partial": every inverse of (omega + i eta) I - H(k) taken for this copy of the
        series -- rule scans, store-free sums, AutoPTR and IAI solves -- pivots by rows, as LAPACK's does.  Rules built
        before the call follow it too; update() keeps it."""
        if mode not in PIVOTING_MODES:
            raise ValueError(f"pivoting must be one of {sorted(PIVOTING_MODES)}, not {mode!r}")
        L.check(L.lib().abz_series_set_pivoting(self.h, PIVOTING_MODES[mode]))

    def pivoting(self):
        m = C.c_int(0)
        L.check(L.lib().abz_series_get_pivoting(self.h, C.byref(m)))
        return {v: k for k, v in PIVOTING_MODES.items()}[m.value]

    # ---- arbitrary nodes (BatchIntegrand body / fallback evaluator)
    def eval_nodes(self, k, want=L.WANT_H):
        k = np.ascontiguousarray(np.asarray(k, dtype=np.float64).reshape(-1, self.s.d))
        nk = len(k)
        n = self.s.n
        H = np.empty((nk, n * n, 2)) if want & L.WANT_H else None
        E = np.empty((nk, n)) if want & L.WANT_EIG else None
        pk = k.ctypes.data_as(L.c_f64p)
        pH = H.ctypes.data_as(L.c_f64p) if H is not None else None
        pE = E.ctypes.data_as(L.c_f64p) if E is not None else None
        # (row-major matrices straight from the device: transposing the reference's column-major blocks here cost more than
        # evaluating them -- 4 096 matrices of 32 x 32: tens of ms)
        L.check(L.lib().abz_eval_nodes(self.h, pk, nk, want | (L.WANT_H_ROW_MAJOR if H is not None else 0), pH, pE))
        out = []
        if H is not None:
            Hc = H.view(np.complex128).reshape(nk, n, n)
            out.append(Hc[:, 0, 0] if self.s.scalar else Hc)
        if E is not None:
            out.append(E)
        return out[0] if len(out) == 1 else tuple(out)

    # ---- IAI building blocks: what abz_iai_solve is built from, for a caller that keeps its own adaptive loop (the
    # semantics of julia/AutoBZCoreHIP.jl's contract_nodes / eval_line_nodes / release_level!)
    def contract_nodes(self, src_level, parents, x):
        """Contract the outermost remaining variable of the level-`src_level` sets `parents` (slot 0 at level d = the
        series itself) at the coordinates `x`, one parent per node (abz_contract_nodes).  Returns the slots of the new
        level-(src_level - 1) sets: consecutive numbers from the level's current count; they stay valid until
        release_level, an IAI solve or update()."""
        parents = np.ascontiguousarray(np.asarray(parents, dtype=np.int64).reshape(-1))
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
        if len(parents) != len(x):
            raise ValueError("contract_nodes: one parent per node")
        slots = np.empty(len(x), dtype=np.int64)
        L.check(L.lib().abz_contract_nodes(self.h, int(src_level), parents.ctypes.data_as(L.c_i64p), x.ctypes.data_as(L.c_f64p),
                                           len(x), slots.ctypes.data_as(L.c_i64p)))
        return slots

    def eval_line_nodes(self, parents, x, integrand, params, sweep, tail=None):
        """Values of the built-in integrand `integrand` at the innermost nodes `x` of the level-1 sets `parents` (all 0
        for d = 1) as complex [nnodes, ncomp] (abz_eval_line_nodes); F_GLOC's n x n matrix comes column-major like
        everywhere in the ABI.  `tail` [nnodes, d - 1]: the outer coordinates x_2..x_d of every node's line, read by
        F_LINEAR_X only."""
        s = self.s
        parents = np.ascontiguousarray(np.asarray(parents, dtype=np.int64).reshape(-1))
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
        if len(parents) != len(x):
            raise ValueError("eval_line_nodes: one parent per node")
        ptail = None
        if tail is not None and s.d > 1:
            tail = np.ascontiguousarray(np.asarray(tail, dtype=np.float64).reshape(-1, s.d - 1))
            if len(tail) != len(x):
                raise ValueError(f"eval_line_nodes: tail of shape {tail.shape}, expected [{len(x)}, {s.d - 1}]")
            ptail = tail.ctypes.data_as(L.c_f64p)
        ncomp = {L.F_GLOC: s.n * s.n, L.F_LINEAR_X: s.d}.get(integrand, 1)
        params = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
        vals = np.empty((len(x), ncomp, 2))
        L.check(L.lib().abz_eval_line_nodes(self.h, parents.ctypes.data_as(L.c_i64p), x.ctypes.data_as(L.c_f64p), ptail, len(x),
                                            int(integrand), params.ctypes.data_as(L.c_f64p) if len(params) else None, len(params),
                                            float(0.0 if sweep is None else sweep), vals.ctypes.data_as(L.c_f64p)))
        return vals.view(np.complex128).reshape(len(x), ncomp)

    def release_level(self, level):
        """Drop every contracted set below `level` (abz_release_level): their slots are invalid from here on."""
        L.check(L.lib().abz_release_level(self.h, int(level)))

    # ---- store-free rule values
    stream_above_bytes = 32 << 30  # rules beyond this many bytes are summed on the fly instead of being cached

    def ptr_sum_supported(self, npt, fid):
        s = self.s
        if fid in (L.F_DOS, L.F_TRGLOC, L.F_GLOC) and self.pivoting() == "partial":
            return npt < 65536  # the pivoted inverse of every node, 1...64 bands
        if s.n > 4:  # generic-n kernels: resolvent traces of Hermitian series from the tridiagonal form; G, and series that are not Hermitian, from the inverse of every node
            if fid in (L.F_DOS, L.F_TRGLOC) and self.hermitian():
                return True
            return fid in (L.F_DOS, L.F_TRGLOC, L.F_GLOC)
        return (npt > 128 and self.hermitian() and
                not (fid in (L.F_LINEAR, L.F_LINEAR_X) and s.n != 1))

    def hermitian(self):
        """H_{-R} = H_R^dagger on the stored coefficient array (what the library detects at upload); cached per
        coefficient generation."""
        cached = getattr(self, "_herm", None)
        if cached is not None and cached[0] == self.generation and cached[1] is self.s.c:
            return cached[2]
        v = self._hermitian_now()
        self._herm = (self.generation, self.s.c, v)
        return v

    def _hermitian_now(self):
        c = self.s.c
        flip = c[tuple(slice(None, None, -1) for _ in range(self.s.d))]
        sym = all(2 * f + m - 1 == 0 for f, m in zip(np.atleast_1d(self.s.first), c.shape[:self.s.d]))
        return bool(sym and np.array_equal(c, np.conj(np.swapaxes(flip, -1, -2))))

    def ptr_sum(self, npt, fid, params=(), sweep=None, nsyms=1):
        """rule(f, B) on the full npt^d grid without materialising H(k) (abz_ptr_sum); with `kshard` set, this
        rank's slab followed by the all-reduce.  Returns complex [n_sweep, ncomp] like DeviceRule.reduce."""
        s = self.s
        ncomp = {L.F_GLOC: s.n * s.n, L.F_LINEAR_X: s.d}.get(fid, 1)
        params = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
        swept = fid in (L.F_DOS, L.F_TRGLOC, L.F_GLOC, L.F_DOS_EIG)
        if swept:
            sw = np.ascontiguousarray(np.asarray(sweep, dtype=np.float64).reshape(-1))
            ns, psw = len(sw), sw.ctypes.data_as(L.c_f64p)
        else:
            ns, psw = 1, None
        out = np.zeros((ns, ncomp, 2))
        z0, z1 = 0, int(npt)
        if self.kshard and self.kshard[1] > 1:
            z0, z1 = slab_range(int(npt), *self.kshard)
        if z1 > z0:
            L.check(L.lib().abz_ptr_sum(self.h, int(npt), z0, z1, fid, params.ctypes.data_as(L.c_f64p) if len(params) else None,
                                        len(params), psw, ns, int(nsyms), out.ctypes.data_as(L.c_f64p)))
        if self.kshard and self.kshard[1] > 1:
            out = self.allreduce(out)
        return out.view(np.complex128).reshape(ns, ncomp)

    # ---- cached PTR rules
    def rule(self, npt, syms=None, want=L.WANT_H):
        """Cached rule.  With `self.kshard = (rank, world)` set (dist.kshard) the rule holds this rank's
        share of the nodes only -- a slab of the outermost variable of a full grid, or every world-th
        irreducible node -- and its reductions are summed over the ranks by `self.allreduce`."""
        # rules of a Hermitian series keep H(k) as its upper triangle (n^2 planes instead of 2 n^2: every built-in
        # integrand reads those planes only, export() still returns full matrices); ABZ_RULE_COMPACT=0: the reference's
        # full SMatrix layout
        want = self._layout_want(want)
        key = (int(npt), _syms_key(syms), int(want), self.kshard)
        r = self.rules.pop(key, None)
        if r is None:
            # a cached superset also serves
            for (n2, s2, w2, k2), r2 in list(self.rules.items()):
                if n2 == key[0] and s2 == key[1] and self._serves(w2, want) and k2 == self.kshard:
                    r = self.rules.pop((n2, s2, w2, k2))
                    key = (n2, s2, w2, k2)
                    break
        if r is None:
            r = DeviceRule(self, npt, syms, want)
            self.rule_bytes += r.nbytes
            while self.rule_bytes > self.max_rule_bytes and self.rules:
                old_key = next(iter(self.rules))
                old = self.rules.pop(old_key)
                self.rule_bytes -= old.nbytes
                old.close()
        self.rules[key] = r  # most recently used last
        return r

    def has_rule(self, npt, syms=None, want=L.WANT_H):
        """Is a rule serving this request already resident?"""
        k0, k1, want = int(npt), _syms_key(syms), self._layout_want(want)
        return any(n2 == k0 and s2 == k1 and self._serves(w2, want) and k2 == self.kshard for (n2, s2, w2, k2) in self.rules)

    def _layout_want(self, want):
        # (1...16 bands; the library ignores the bit where it has no upper-triangle kernel and reports the layout it built)
        if (want & L.WANT_H) and self.s.n <= 16 and os.environ.get("ABZ_RULE_COMPACT", "1") != "0" and self.hermitian():
            want |= L.WANT_H_COMPACT
        return int(want)

    @staticmethod
    def _serves(have, want):
        """A cached rule with planes `have` serves a request for `want`: every requested plane family is there and, when
        H planes are requested, in the requested layout (full SMatrix order or upper triangle) -- a zero-copy client of
        values_ptr must not be handed the other one."""
        return (have & want) == want and (not (want & L.WANT_H) or (have & L.WANT_H_COMPACT) == (want & L.WANT_H_COMPACT))

    def drop_rules(self):
        for r in self.rules.values():
            r.close()
        self.rules.clear()
        self.rule_bytes = 0
        if self._h is not None:  # ... and the rules the library keeps for its whole-solve entry points
            L.check(L.lib().abz_series_drop_rules(self.h))


def slab_range(n, rank, world):
    """Balanced contiguous share [a, b) of range(n) for `rank` of `world`."""
    return (n * rank) // world, (n * (rank + 1)) // world


def _syms_key(syms):
    if syms is None:
        return None
    return np.ascontiguousarray(np.rint(np.asarray(syms)).astype(np.int32)).tobytes()


def symptr_rule(npt, d, syms, ctx=None):
    """Irreducible grid nodes (0-based indices, column-major order) and integer weights.
    ref: AutoSymPTR.symptr_rule as called at src/fourier.jl:271.  With a device context the orbit
    tables are computed on the GPU (abz_symptr_rule_device), otherwise by the host routine; both give
    bit-identical integers."""
    S = np.ascontiguousarray(np.rint(np.asarray(syms)).astype(np.int32).reshape(-1, d, d))
    if not np.allclose(S, np.asarray(syms).reshape(-1, d, d)):
        raise ValueError("symmetries must be integer matrices in the lattice basis")
    _, pS = L.i32(S)
    n = C.c_int64(0)
    if ctx is not None and len(S) <= 48:
        fn = lambda *a: L.lib().abz_symptr_rule_device(ctx.h, *a)
    else:
        fn = L.lib().abz_symptr_rule
    L.check(fn(npt, d, pS, len(S), C.byref(n), None, None))
    idx = np.empty((n.value, d), dtype=np.int32)
    w = np.empty(n.value, dtype=np.int64)
    L.check(fn(npt, d, pS, len(S), C.byref(n), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p)))
    return idx, w


def density_matrix_orbitals(orbitals, n, who="ltm_density_matrix"):
    """The orbital selection of a density matrix as an index array (None: all n); ValueError as in ltm_green_matrix, and for an
    index outside 0..n-1 (the sub-block is cut on the host: no device call would refuse it)."""
    orb = np.arange(n) if orbitals is None else np.asarray(orbitals).reshape(-1)
    if orb.size < 1 or not np.issubdtype(orb.dtype, np.integer):
        raise ValueError(f"{who}: orbitals = {orbitals!r} is not a sequence of orbital indices")
    if len(set(orb.tolist())) != len(orb):
        raise ValueError(f"{who}: orbitals = {orbitals!r} names an orbital twice")
    if orb.min() < 0 or orb.max() >= n:
        raise ValueError(f"{who}: orbitals = {orbitals!r} outside 0..{n - 1}")
    return orb


def expectation_components(components, nops, who="ltm_expectation"):
    """The components of one band-expectation call as an int32 array [ncomp, 2] -- (i, -1): q_i, (i, j): q_i q_j -- or None for
    the nops expectations in order; ValueError, before the library is called, for none or more than 16 of them, an entry
    that is neither an index nor a pair, and an operator index outside 0..nops-1."""
    if components is None:
        return None
    out = []
    for c in components:
        pair = (c, -1) if np.ndim(c) == 0 else tuple(c)
        if len(pair) != 2 or not all(isinstance(v, (int, np.integer)) for v in pair):
            raise ValueError(f"{who}: component {c!r} is neither an operator index nor a pair of them")
        i, j = int(pair[0]), int(pair[1])
        if not (0 <= i < nops and -1 <= j < nops):
            raise ValueError(f"{who}: component {c!r} names an operator outside 0..{nops - 1}")
        out.append((i, j))
    if not 1 <= len(out) <= L.LTM_MAX_COMP:
        raise ValueError(f"{who}: {len(out)} components, a call takes 1..{L.LTM_MAX_COMP}")
    return np.ascontiguousarray(np.array(out, dtype=np.int32).reshape(-1, 2))


def green_node_weight_zs(zs, who="ltm_green_node_weights"):
    """The values of z of one complex-weight call as a complex128 array; ValueError, before the library is called, for none or
    more than 8 of them and for a real or non-finite one."""
    zs = np.ascontiguousarray(np.asarray(zs, dtype=np.complex128).reshape(-1))
    if not 1 <= len(zs) <= L.LTM_GREEN_NODEW_MAX_Z:
        raise ValueError(f"{who}: {len(zs)} values of z, a call takes 1..{L.LTM_GREEN_NODEW_MAX_Z}")
    if not (np.all(np.isfinite(zs.real)) and np.all(np.isfinite(zs.imag))):
        raise ValueError(f"{who}: zs = {zs!r} holds a value that is not finite")
    if np.any(zs.imag == 0.0):
        raise ValueError(f"{who}: zs = {zs!r} holds a real value; G is computed off the real axis (Im z != 0)")
    return zs


def band_range(r, who, name):
    """A band range given as a `range` (step 1) or (start, count) -> (start, count); ValueError otherwise."""
    if isinstance(r, range):
        if r.step != 1 or len(r) < 1:
            raise ValueError(f"{who}: {name} = {r!r} is not a non-empty range of consecutive bands")
        return int(r.start), len(r)
    try:
        start, count = r
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} = {r!r} is neither a range nor (start, count)") from None
    if not all(isinstance(v, (int, np.integer)) for v in (start, count)) or start < 0 or count < 1:
        raise ValueError(f"{who}: {name} = {r!r} is neither a range nor (start, count) with start >= 0, count >= 1")
    return int(start), int(count)


def pair_ranges(lower, upper, n=None, who="ltm_pairs"):
    """(v0, nv, c0, nc) of a lower and an upper band range; ValueError, before the library is called, for ranges that overlap
    or are out of order, that leave the n bands, or that make more than 64 pairs."""
    v0, nv = band_range(lower, who, "lower")
    c0, nc = band_range(upper, who, "upper")
    if v0 + nv > c0:
        raise ValueError(f"{who}: the lower bands [{v0}, {v0 + nv}) must lie below the upper bands [{c0}, {c0 + nc})")
    if n is not None and c0 + nc > n:
        raise ValueError(f"{who}: the upper bands [{c0}, {c0 + nc}) leave the {n} bands of the series")
    if nv * nc > L.MAX_BANDS:
        raise ValueError(f"{who}: {nv} x {nc} = {nv * nc} pairs, a pair rule takes {L.MAX_BANDS}; take a window of bands around the gap")
    return v0, nv, c0, nc


def pair_components(components, nops, who="ltm_pairs"):
    """The components of a pair rule as an int32 array [ncomp, 3] -- (i, j, part): Re (0) or Im (1) of M^i conj(M^j) -- or None
    for |M^i|^2 of the nops operators in order.  Entries: i, (i, j) or (i, j, "re" | "im"); ValueError, before the library is
    called, for none or more than 16 of them, a malformed entry and an operator index outside 0..nops-1."""
    if components is None:
        return None
    out = []
    for c in components:
        t = (c, c, "re") if np.ndim(c) == 0 else tuple(c)
        if len(t) == 2:
            t = (t[0], t[1], "re")
        if len(t) != 3 or not all(isinstance(v, (int, np.integer)) for v in t[:2]) or t[2] not in ("re", "im"):
            raise ValueError(f"{who}: component {c!r} is neither an operator index i, a pair (i, j) nor (i, j, 're' | 'im')")
        i, j = int(t[0]), int(t[1])
        if not (0 <= i < nops and 0 <= j < nops):
            raise ValueError(f"{who}: component {c!r} names an operator outside 0..{nops - 1}")
        out.append((i, j, 0 if t[2] == "re" else 1))
    if not 1 <= len(out) <= L.LTM_MAX_COMP:
        raise ValueError(f"{who}: {len(out)} components, a call takes 1..{L.LTM_MAX_COMP}")
    return np.ascontiguousarray(np.array(out, dtype=np.int32).reshape(-1, 3))


class DeviceRule:
    """abz_rule handle: FourierPTR (syms None) or FourierMonkhorstPack values resident in HBM.
    ref: src/fourier.jl:127-174,210-277."""

    def __init__(self, dev: DeviceSeries, npt, syms, want):
        self.dev = dev
        self.npt = int(npt)
        self.want = int(want)
        self.syms = syms
        self.nsyms = 1 if syms is None else len(syms)
        h = C.c_void_p()
        d, n = dev.s.d, dev.s.n
        self.shard = dev.kshard
        rank, world = self.shard if self.shard else (0, 1)
        if syms is None:
            self.nk = self.npt ** d  # nodes of the whole rule (numevals counts these)
            if world == 1:
                L.check(L.lib().abz_ptr_rule_build(dev.h, self.npt, 0, None, None, want, C.byref(h)))
                self.nk_local = self.nk
            else:
                if d < 2:
                    raise ValueError("k-sharding needs at least two variables")
                z0, z1 = slab_range(self.npt, rank, world)
                self.nk_local = (z1 - z0) * self.npt ** (d - 1)
                if z1 > z0:
                    L.check(L.lib().abz_ptr_rule_build_slab(dev.h, self.npt, z0, z1, want, C.byref(h)))
        elif world == 1 and len(syms) <= 48 and os.environ.get("ABZ_SYM_DEVICE", "1") != "0":
            # orbit tables, contraction plan and values all on the device (abz_ptr_rule_build_sym): the node list
            # never visits the host
            S = np.ascontiguousarray(np.rint(np.asarray(syms)).astype(np.int32).reshape(-1, d, d))
            if not np.allclose(S, np.asarray(syms).reshape(-1, d, d)):
                raise ValueError("symmetries must be integer matrices in the lattice basis")
            L.check(L.lib().abz_ptr_rule_build_sym(dev.h, self.npt, S.ctypes.data_as(L.c_i32p), len(S), want, C.byref(h)))
            nk = C.c_int64(0)
            L.check(L.lib().abz_rule_info(h, C.byref(nk), None, None, None, None))
            self.nk = self.nk_local = int(nk.value)
        else:
            idx, w = symptr_rule(self.npt, d, syms, ctx=dev.ctx)
            self.nk = len(w)
            if world > 1:  # consecutive blocks keep the runs of shared outer coordinates together
                a, b = slab_range(len(w), rank, world)
                idx, w = np.ascontiguousarray(idx[a:b]), np.ascontiguousarray(w[a:b])
            self.nk_local = len(w)
            if len(w):
                L.check(L.lib().abz_ptr_rule_build(dev.h, self.npt, len(w), idx.ctypes.data_as(L.c_i32p),
                                                   w.ctypes.data_as(L.c_i64p), want, C.byref(h)))
        self._adopt(h)
        if self._h is not None and want & L.WANT_H_COMPACT:  # the library drops the bit when the layout does not apply
            got = C.c_int(0)
            L.check(L.lib().abz_rule_info(self._h, None, None, None, None, C.byref(got)))
            self.want = want = int(got.value)
        per = ((n * n if want & L.WANT_H_COMPACT else 2 * n * n) if want & L.WANT_H else 0) + (n if want & (L.WANT_EIG | L.WANT_VEL) else 0) + \
              (d * n if want & L.WANT_VEL else 0)
        self.nbytes = 8 * per * self.nk_local

    def _adopt(self, h):
        """The state every rule object keeps about its handle (subclasses that make the handle another way call this too)."""
        self._h = h if h.value else None
        self._closed = False
        self._ltm_ncomp = 0  # components of the matrix elements attached by ltm_elements
        self._ltm_halo = False  # a k-sharded rule: ltm_halo() made its slab scannable
        self.generation = self.dev.generation
        self._fin = weakref.finalize(self, DeviceRule._destroy, self._h)

    @property
    def h(self):
        """The abz_rule handle (None for an empty k-shard); a stale rule is refilled first, and an attached halo plane
        (ltm_halo) with it: abz_rule_rebuild does both."""
        if self._closed:
            raise L.AbzError("DeviceRule was closed")
        if self._h is not None and self.generation != self.dev.generation:
            self.generation = self.dev.generation
            self._ltm_ncomp = 0  # the library drops attached matrix elements with the old eigenstates
            L.check(L.lib().abz_rule_rebuild(self._h))
        return self._h

    @staticmethod
    def _destroy(h):
        try:
            if h is not None:
                L.lib().abz_rule_destroy(h)
        except Exception:
            pass

    def _sum_over_ranks(self, a):
        """Partial sums of this rank's share -> the value of the whole rule (the all-reduce of a
        k-sharded solve)."""
        return self.dev.allreduce(a) if self.shard and self.shard[1] > 1 else a

    def close(self):
        self._fin()
        self._closed = True
        self._h = None

    def __len__(self):
        return self.nk

    @property
    def nbands(self):
        """Bands of the rule's eigenvalue planes, attached elements and weight blocks (abz_rule_ltm_bands): the series' n, or
        the nv nc pseudo-bands of a PairRule."""
        if self._h is None:
            return self.dev.s.n
        nb = C.c_int(0)
        L.check(L.lib().abz_rule_ltm_bands(self._h, C.byref(nb)))
        return int(nb.value)

    def rebuild(self):
        """Re-evaluate all cached values in place from the series' current coefficients (async)."""
        if self._closed:
            raise L.AbzError("DeviceRule was closed")
        if self._h is not None:
            self.generation = self.dev.generation
            self._ltm_ncomp = 0
            L.check(L.lib().abz_rule_rebuild(self._h))

    def reduce(self, fid, params=(), sweep=None, nsyms=None):
        """(sum_k w_k f(k, H(k); sweep_i)) / (npt^d nsyms) for every sweep value -> complex array
        [n_sweep, ncomp].  ref: rule(f, B) = quadsum(...), src/fourier.jl:204-207,289-292."""
        s = self.dev.s
        ncomp = {L.F_GLOC: s.n * s.n, L.F_LINEAR_X: s.d}.get(fid, 1)
        params = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
        swept = fid in (L.F_DOS, L.F_TRGLOC, L.F_GLOC, L.F_DOS_EIG)
        if swept:
            sw = np.ascontiguousarray(np.asarray(sweep, dtype=np.float64).reshape(-1))
            ns = len(sw)
            psw = sw.ctypes.data_as(L.c_f64p)
        else:
            ns, psw = 1, None
        out = np.zeros((ns, ncomp, 2))
        pp = params.ctypes.data_as(L.c_f64p) if len(params) else None
        if self.h is not None:
            L.check(L.lib().abz_rule_reduce(self.h, fid, pp, len(params), psw, ns,
                                            self.nsyms if nsyms is None else nsyms, out.ctypes.data_as(L.c_f64p)))
        return self._sum_over_ranks(out).view(np.complex128).reshape(ns, ncomp)

    def reduce_device(self, fid, params, sweep_ptr, n_sweep, out_ptr, nsyms=None):
        """abz_rule_reduce_device: `sweep_ptr` / `out_ptr` are raw device addresses (e.g. tensor.data_ptr()) of
        [n_sweep] and [n_sweep][ncomp][2] doubles; enqueues on the context's stream and returns.  The caller
        follows with its collective on the same stream (dist.py)."""
        params = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
        pp = params.ctypes.data_as(L.c_f64p) if len(params) else None
        if self.h is not None:
            L.check(L.lib().abz_rule_reduce_device(self.h, fid, pp, len(params), C.c_void_p(int(sweep_ptr)), int(n_sweep),
                                                   self.nsyms if nsyms is None else nsyms, C.c_void_p(int(out_ptr))))

    def values_ptr(self):
        """(device address, bytes) of the rule's value block."""
        base = C.c_void_p()
        nb = C.c_int64(0)
        L.check(L.lib().abz_rule_values_ptr(self.h, C.byref(base), C.byref(nb)))
        return int(base.value or 0), int(nb.value)

    def export(self, x=True, w=True, H=False, eig=False, vel=False):
        """Host copies in the reference's layout: x [nk,d], w [nk], H [nk,n,n], eig [nk,n], vel [nk,d,n]."""
        s = self.dev.s
        nk, n, d = self.nk_local, s.n, s.d  # a k-sharded rule exports this rank's nodes
        X = np.empty((nk, d)) if x else None
        W = np.empty(nk) if w else None
        Hb = np.empty((nk, n * n, 2)) if H else None
        E = np.empty((nk, self.nbands)) if eig else None
        V = np.empty((nk, d, n)) if vel else None
        ptr = lambda a: a.ctypes.data_as(L.c_f64p) if a is not None else None
        if self.h is not None:
            L.check(L.lib().abz_rule_export(self.h, ptr(X), ptr(W), ptr(Hb), ptr(E), ptr(V)))
        out = {}
        if x:
            out["x"] = X
        if w:
            out["w"] = W
        if H:
            Hc = Hb.view(np.complex128).reshape(nk, n, n).transpose(0, 2, 1)
            out["H"] = Hc[:, 0, 0] if s.scalar else np.ascontiguousarray(Hc)
        if eig:
            out["eig"] = E
        if vel:
            out["vel"] = V
        return out

    def ggr(self, Es):
        """sum_k w_k sum_bands ggr_formula(1/(2 npt), E, e, v...).  ref: src/dos_ggr.jl:58-65."""
        Es = np.ascontiguousarray(np.asarray(Es, dtype=np.float64).reshape(-1))
        out = np.zeros(len(Es))
        if self.h is not None:
            L.check(L.lib().abz_rule_ggr(self.h, Es.ctypes.data_as(L.c_f64p), len(Es), out.ctypes.data_as(L.c_f64p)))
        return self._sum_over_ranks(out)

    def _ltm_refuse_shard(self, what=None):
        """Everything of LTM but the scans of `ltm` refuses a k-sharded rule; `what` names the caller once a halo is there."""
        if self.shard and self.shard[1] > 1:
            if self._ltm_halo and what:
                raise NotImplementedError(f"{what} on a k-sharded (slab) rule is not implemented: with its halo plane a slab serves "
                                          "ltm(Es) and ltm(Es, elements='energy') only")
            raise NotImplementedError("LTM on a k-sharded (slab) rule is not implemented: the simplices of a slab's last "
                                      "plane need one halo plane from the next rank")

    def ltm_halo(self):
        """Make this rank's slab of a k-sharded full-grid rule scannable by `ltm` (abz_rule_ltm_halo): the rule computes the
        one plane behind its slab itself, eigenvalues only, 1/npt of the grid and no exchange between ranks.  The plane
        belongs to the rule: it is refilled with it when the series changes and goes with it.  Nothing to do on a rank whose
        slab is empty; ValueError on a rule that is not sharded."""
        if not (self.shard and self.shard[1] > 1):
            raise ValueError("ltm_halo: the rule is not k-sharded (a whole grid needs no halo plane)")
        if self.syms is not None:
            raise NotImplementedError("ltm_halo: a k-sharded symmetric rule holds a block of irreducible nodes, not a slab of the grid")
        h = self.h  # (a stale rule is refilled here)
        if h is not None:
            L.check(L.lib().abz_rule_ltm_halo(h))
            if not self._ltm_halo:
                add = 8 * self.dev.s.n * self.npt ** (self.dev.s.d - 1)
                self.nbytes += add
                if any(r is self for r in self.dev.rules.values()):
                    self.dev.rule_bytes += add
        self._ltm_halo = True

    def ltm_elements(self, A):
        """Attach matrix elements A [ncomp, nk, n] (node and band order of export()'s eig [nk, n]) to the rule for
        weighted tetrahedron scans (abz_rule_ltm_elements); `None` drops them.  They stay on the device until replaced,
        dropped, or the rule is rebuilt."""
        self._ltm_refuse_shard("ltm_elements")
        if A is None:
            L.check(L.lib().abz_rule_ltm_elements(self.h, None, 0))
            self._ltm_ncomp = 0
            return
        s = self.dev.s
        A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
        if A.ndim == 2:
            A = A[None]
        if A.ndim != 3 or A.shape[1:] != (self.nk, self.nbands):
            raise ValueError(f"ltm_elements: elements of shape {A.shape}, expected [ncomp, {self.nk}, {self.nbands}]")
        L.check(L.lib().abz_rule_ltm_elements(self.h, A.ctypes.data_as(L.c_f64p), A.shape[0]))
        self._ltm_ncomp = A.shape[0]

    def ltm_orbitals(self, orbitals=None):
        """Attach the orbital weights |U_ab(k)|^2 as matrix elements, computed on the device from H(k)
        (abz_rule_ltm_orbitals): component c is orbital `orbitals[c]` (None: all n <= 16 of them), bands ascending as in
        export()'s eig.  H(k) comes from the rule, or from a transient rule when it keeps eigenvalues only.  At a degenerate
        level the weights belong to some orthonormal basis of the eigenspace.  `ltm(Es, elements="attached")` scans them."""
        self._ltm_refuse_shard("ltm_orbitals")
        h = self.h  # (a stale rule is refilled here)
        if orbitals is None:
            L.check(L.lib().abz_rule_ltm_orbitals(h, None, 0))
            self._ltm_ncomp = self.dev.s.n
            return
        orb = np.ascontiguousarray(np.asarray(orbitals).reshape(-1))
        if orb.size and not np.issubdtype(orb.dtype, np.integer):
            raise ValueError(f"ltm_orbitals: orbitals = {orbitals!r} are not integer indices")
        orb = orb.astype(np.int32)
        L.check(L.lib().abz_rule_ltm_orbitals(h, orb.ctypes.data_as(L.c_i32p), len(orb)))
        self._ltm_ncomp = len(orb)

    def ltm_projectors(self, pairs):
        """Attach the band projectors P^b_pq(k) = U_pb(k) conj(U_qb(k)) of the orbital pairs `pairs` [npairs, 2] as matrix
        elements, computed on the device like the orbital weights (abz_rule_ltm_projectors).  A pair (p, p) is one component,
        |U_pb|^2; a pair p != q is two, Re P then Im P; at most 16 components in all, in the order of the pairs.  No phase of
        an eigenvector changes them; at a degenerate level they belong to some orthonormal basis of the eigenspace and only
        their sum over the level is defined.  `ltm_green(zs, elements="attached")` then gives G_{Re P} and G_{Im P}, and
        G_pq = G_{Re P} + i G_{Im P}, G_qp = G_{Re P} - i G_{Im P} (`ltm_green_matrix` does that)."""
        self._ltm_refuse_shard("ltm_projectors")
        h = self.h  # (a stale rule is refilled here)
        pr = np.asarray(pairs)
        if pr.size and not np.issubdtype(pr.dtype, np.integer):
            raise ValueError(f"ltm_projectors: pairs = {pairs!r} are not integer indices")
        if pr.ndim != 2 or pr.shape[1] != 2:
            raise ValueError(f"ltm_projectors: pairs of shape {pr.shape}, expected [npairs, 2]")
        pr = np.ascontiguousarray(pr.astype(np.int32))
        L.check(L.lib().abz_rule_ltm_projectors(h, pr.ctypes.data_as(L.c_i32p), len(pr)))
        self._ltm_ncomp = int(np.where(pr[:, 0] == pr[:, 1], 1, 2).sum())

    def _operator_rules(self, ops, who):
        """The operators of `ltm_expectation` / `ltm_pairs` as rules with H planes on this rule's grid: a FourierSeries through
        its copy on this rule's context and that copy's cached rule(npt, None, WANT_H), a DeviceRule as it is."""
        rules = []
        for i, op in enumerate(ops):
            if isinstance(op, FourierSeries):
                op = op.device(self.dev.ctx).rule(self.npt, None, L.WANT_H)
            elif not isinstance(op, DeviceRule):
                raise ValueError(f"{who}: operators[{i}] = {op!r} is neither a FourierSeries nor a DeviceRule")
            rules.append(op)
        return rules

    def ltm_expectation(self, operators, components=None):
        """Attach band expectation values of operator series as matrix elements, computed on the device from H(k) and the
        operators' values on the same grid (abz_rule_ltm_expectation): q_i = Re u_b^H Hermitian(O_i(k)) u_b for operator i, band b
        (ascending as in export()'s eig) and node k, the upper triangle of O_i read the way H is.  `operators`: 1..8 of them,
        each a FourierSeries in the Wannier basis of H (its copy on this rule's context and that copy's cached
        rule(npt, None, WANT_H) are used) or a DeviceRule that holds H planes of the same grid (this rule itself when it holds
        H: q = e_b); the caller keeps such rules current.  `components`: None for the expectations in order, or a sequence of
        at most 16 entries, each an operator index i (q_i) or a pair (i, j) (the product q_i q_j; (i, -1) is q_i): with
        O_a = h.derivative(a) and all pairs, `ltm(Es, elements="attached")` is the transport distribution
        sum_b int dk v_a v_b delta(E - e_b).  At a degenerate level single expectations belong to some orthonormal basis of
        the eigenspace: only their sum over the level is defined, products are not defined there.
        Measured on an MI355X (tools/time_ltm_expectation.py, profiles/ltm_expectation.txt; 3 operators, 6 components, medians
        of 7, the operator rules resident): 3 bands 48^3 0.063 ms on a rule of eigenvalues only and 0.042 ms on a rule with H
        (kernel 0.019 ms), the host route -- export H and the operator planes, numpy.linalg.eigh, einsum, ltm_elements --
        193 ms; 16 bands 24^3 0.352 / 0.290 ms (kernel 0.260) against 757 ms; 32 bands 16^3 0.659 / 0.565 ms (kernel 0.536)
        against 1188 ms.  ltm_orbitals with 6 components on the same rules: 0.049 / 0.027, 0.247 / 0.180 and 0.413 / 0.349 ms
        -- the three operators cost about 0.6 times the eigen-solve they ride on."""
        self._ltm_refuse_shard("ltm_expectation")
        ops = list(operators) if isinstance(operators, (list, tuple)) else [operators]
        if not 1 <= len(ops) <= L.LTM_EXPECT_MAX_OPS:
            raise ValueError(f"ltm_expectation: {len(ops)} operators, a call takes 1..{L.LTM_EXPECT_MAX_OPS}")
        comps = expectation_components(components, len(ops), "ltm_expectation")
        h = self.h  # (a stale rule is refilled here)
        rules = self._operator_rules(ops, "ltm_expectation")
        handles = (C.c_void_p * len(rules))(*[getattr(r.h, "value", None) for r in rules])  # (stale operator rules are refilled here)
        L.check(L.lib().abz_rule_ltm_expectation(h, handles, len(rules), None if comps is None else comps.ctypes.data_as(L.c_i32p),
                                                 len(rules) if comps is None else len(comps)))
        self._ltm_ncomp = len(rules) if comps is None else len(comps)

    def ltm_green_matrix(self, zs, orbitals=None):
        """The local Green's function G_pq(z) = sum_b int dk U_pb conj(U_qb) / (z - e_b(k)) on the orbitals `orbitals` (None:
        all n) at the complex energies `zs` (Im z != 0), per unit cell, complex128 [nz, m, m]: the tetrahedron counterpart of a
        grid mean of inv(z - H(k)), with the interpolation error O(1/npt^2) whatever Im z is.  The m diagonal pairs and the
        m (m - 1) / 2 pairs p < q are dealt, in that order, into groups of at most 16 components (one for a diagonal pair, two
        for the others; m <= 4 is one group); every group is attached with `ltm_projectors` and scanned with
        `ltm_green(zs, elements="attached")`.  Each group repeats the eigen-solve of the whole grid: the eigenvectors are
        never stored.  The last group stays attached, and a DOS cache on the same rule attaches its own elements again."""
        self._ltm_refuse_shard("ltm_green_matrix")
        zs = np.ascontiguousarray(np.asarray(zs, dtype=np.complex128).reshape(-1))
        n = self.dev.s.n
        orb = np.arange(n) if orbitals is None else np.asarray(orbitals).reshape(-1)
        if orb.size < 1 or not np.issubdtype(orb.dtype, np.integer):
            raise ValueError(f"ltm_green_matrix: orbitals = {orbitals!r} is not a sequence of orbital indices")
        if len(set(orb.tolist())) != len(orb):
            raise ValueError(f"ltm_green_matrix: orbitals = {orbitals!r} names an orbital twice")
        m = len(orb)
        todo = [(a, a) for a in range(m)] + [(a, b) for a in range(m) for b in range(a + 1, m)]  # positions in `orb`
        groups, ncomp = [[]], 0
        for a, b in todo:
            need = 1 if a == b else 2
            if ncomp + need > L.LTM_MAX_COMP:
                groups.append([])
                ncomp = 0
            groups[-1].append((a, b))
            ncomp += need
        G = np.zeros((len(zs), m, m), dtype=np.complex128)
        for group in groups:
            self.ltm_projectors([(orb[a], orb[b]) for a, b in group])
            self._ltm_owner = None  # (whatever a DOS cache had attached is gone)
            g = self.ltm_green(zs, elements="attached")
            c = 0
            for a, b in group:
                if a == b:
                    G[:, a, a] = g[:, c]
                    c += 1
                else:
                    G[:, a, b] = g[:, c] + 1j * g[:, c + 1]
                    G[:, b, a] = g[:, c] - 1j * g[:, c + 1]
                    c += 2
        return G

    def ltm_elements_export(self):
        """The attached matrix elements [ncomp, nk, n] back on the host (abz_rule_ltm_elements_export), in the order
        ltm_elements takes them; None when nothing is attached."""
        self._ltm_refuse_shard("ltm_elements_export")
        h = self.h  # (a stale rule is refilled here, which drops the attached elements)
        nc = C.c_int(0)
        L.check(L.lib().abz_rule_ltm_elements_export(h, C.byref(nc), None))
        if nc.value == 0:
            return None
        A = np.empty((nc.value, self.nk, self.nbands))
        L.check(L.lib().abz_rule_ltm_elements_export(h, C.byref(nc), A.ctypes.data_as(L.c_f64p)))
        return A

    def ltm_elements_ptr(self):
        """(device address, bytes, ncomp) of the resident element block (abz_rule_ltm_elements_ptr): double
        [nk / npt, ncomp * nbands, row], row = npt rounded up to a multiple of 16, zeros in the padding columns; (0, 0, 0) when
        nothing is attached."""
        self._ltm_refuse_shard("ltm_elements_ptr")
        return self._ltm_ptr(L.lib().abz_rule_ltm_elements_ptr)

    def _ltm_ptr(self, fn):
        """(device address, bytes, count) of a resident block from its C entry point `fn`."""
        base, nb, count = C.c_void_p(), C.c_int64(0), C.c_int(0)
        L.check(fn(self.h, C.byref(base), C.byref(nb), C.byref(count)))
        return int(base.value or 0), int(nb.value), int(count.value)

    def ltm(self, Es, states=False, elements=None, correction=False):
        """Linear tetrahedron method on the rule's eigenvalues (abz_rule_ltm): the DOS g(E) or, with `states`, the
        number of states N(E) below E, per unit cell and summed over bands.  The rule must be a whole periodic grid, or a
        k-sharded one after `ltm_halo()`: every rank scans the cells of its slab and the partial sums are summed over the
        ranks (`elements` None or "energy" only).

        `elements`: matrix elements A_b(k), interpolated linearly inside a simplex like the energy; the result is then
        g_A(E) = sum_b int A_b delta(E - e_b) or N_A(E) = sum_b int A_b theta(E - e_b) as [nE, ncomp]
        (abz_rule_ltm_weighted).  "energy": A = e itself (one component); "attached": what ltm_elements attached; an
        array [ncomp, nk, n]: attached first.

        `correction` (with `states` and `elements`): N_A with Bloechl's curvature correction (ABZ_LTM_STATES_CORRECTED),
        N_A + w sum_T g_T(E) kappa_T, kappa_T = sum_i A_i (sum_l e_l - (d+1) e_i) / (2 (d+1)(d+2)), in the same launches.  It
        removes the leading O(1/npt^2) error of a sum taken at FIXED FILLING -- at the level `ltm_fermi` finds on the same
        grid; at a fixed energy the misplaced Fermi surface leaves an error of that order (`ltm_optimized` has no such
        limit).  The plain state count has no correction (kappa_T = 0 for A = 1)."""
        sharded = bool(self.shard and self.shard[1] > 1)
        if sharded and not self._ltm_halo:
            self._ltm_refuse_shard()
        if sharded and not (elements is None or (isinstance(elements, str) and elements == "energy")):
            self._ltm_refuse_shard("ltm with attached elements")
        if correction:
            if not states:
                raise ValueError("ltm: correction=True corrects the state sum N_A: it needs states=True (the DOS has no correction)")
            if elements is None:
                raise ValueError("ltm: correction=True needs elements (the correction of the unweighted state count is zero)")
        Es = np.ascontiguousarray(np.asarray(Es, dtype=np.float64).reshape(-1))
        what = L.LTM_STATES_CORRECTED if correction else (L.LTM_STATES if states else L.LTM_DOS)
        if elements is None:
            out = np.zeros(len(Es))
            h = self.h
            if h is not None:  # (an empty slab adds nothing)
                L.check(L.lib().abz_rule_ltm(h, Es.ctypes.data_as(L.c_f64p), len(Es), what, out.ctypes.data_as(L.c_f64p)))
            return self._sum_over_ranks(out)
        if isinstance(elements, str):
            if elements not in ("energy", "attached"):
                raise ValueError(f"ltm: elements = {elements!r} is neither 'energy' nor 'attached'")
        else:
            self.ltm_elements(elements)
            elements = "attached"
        h = self.h  # (a stale rule is refilled here, which drops the attached elements)
        ncomp = 1 if elements == "energy" else self._ltm_ncomp
        if ncomp < 1:
            raise ValueError("ltm: no matrix elements are attached (ltm_elements; a rebuild of the rule drops them)")
        out = np.zeros((len(Es), ncomp))
        if h is not None:
            L.check(L.lib().abz_rule_ltm_weighted(h, L.LTM_A_ENERGY if elements == "energy" else L.LTM_A_ELEMENTS,
                                                  Es.ctypes.data_as(L.c_f64p), len(Es), what, out.ctypes.data_as(L.c_f64p)))
        return self._sum_over_ranks(out)

    def ltm_optimized(self, Es, states=False, elements=None):
        """`ltm(Es, states, elements)` by the optimized tetrahedron method of Kawamura, Gohda and Tsuneyuki, PRB 89, 094515
        (abz_rule_ltm_optimized; d = 3): every simplex takes the band at its 4 corners and at 16 neighbouring grid points and
        replaces the corner values by those of the linear function closest, in the least-squares sense over the simplex, to
        the cubic through the 20 values; the closed forms of `ltm` then apply to these effective corner values.  Same
        eigenvalues, no further eigen-solve, and the error falls like a higher power of 1/npt AT ANY ENERGY: the rule at npt
        compares with the linear rule at 2 npt.  `elements`: None (g, N as [nE]), "energy", "attached" or an array
        [ncomp, nk, n] as for `ltm` ([nE, ncomp]); they take the same 20-point fit.  There is no `correction`: this rule
        replaces it.  NotImplementedError on a k-sharded rule (the stencil needs three halo planes) and for d < 3."""
        self._ltm_refuse_optimized("ltm_optimized")
        Es = np.ascontiguousarray(np.asarray(Es, dtype=np.float64).reshape(-1))
        what = L.LTM_STATES if states else L.LTM_DOS
        if elements is None:
            source, ncomp = L.LTM_A_ONE, 1
        elif isinstance(elements, str):
            if elements not in ("energy", "attached"):
                raise ValueError(f"ltm_optimized: elements = {elements!r} is neither 'energy' nor 'attached'")
            source = L.LTM_A_ENERGY if elements == "energy" else L.LTM_A_ELEMENTS
        else:
            self.ltm_elements(elements)
            source = L.LTM_A_ELEMENTS
        h = self.h  # (a stale rule is refilled here, which drops the attached elements)
        if source == L.LTM_A_ELEMENTS:
            ncomp = self._ltm_ncomp
            if ncomp < 1:
                raise ValueError("ltm_optimized: no matrix elements are attached (ltm_elements; a rebuild of the rule drops them)")
        elif source == L.LTM_A_ENERGY:
            ncomp = 1
        out = np.zeros((len(Es), ncomp))
        L.check(L.lib().abz_rule_ltm_optimized(h, source, Es.ctypes.data_as(L.c_f64p), len(Es), what, out.ctypes.data_as(L.c_f64p)))
        return out[:, 0] if elements is None else out

    def _ltm_refuse_optimized(self, who):
        if self.shard and self.shard[1] > 1:
            raise NotImplementedError(f"{who} on a k-sharded (slab) rule is not implemented: the 20-point stencil of a simplex "
                                      "needs three halo planes")
        if self.dev.s.d != 3:
            raise NotImplementedError(f"{who}: the optimized tetrahedron rule is implemented for d = 3 (the series has d = {self.dev.s.d})")

    def ltm_fermi_optimized(self, nstates, tol=1e-10):
        """(E_F, N(E_F)) as `ltm_fermi` returns them, for the state count of `ltm_optimized`: E_F is the upper end of an
        interval no wider than `tol` with N(E_F) >= nstates (1 - 1e-12) and N below that at its lower end; below a gap it is
        moved up to the lowest energy with g(E_F) = 0.  The search runs on the host and brackets with device scans of 512
        energies each, 511 times narrower per scan: the optimized N is monotone like the linear one (every simplex adds a
        non-decreasing function of E)."""
        self._ltm_refuse_optimized("ltm_fermi_optimized")
        n = self.nbands
        nstates, tol = float(nstates), float(tol)
        if not (0.0 < nstates < n):
            raise ValueError(f"ltm_fermi_optimized: nstates = {nstates} outside (0, {n})")
        if not tol > 0.0:
            raise ValueError(f"ltm_fermi_optimized: tol = {tol} is not positive")
        eig = self.export(x=False, w=False, eig=True)["eig"]
        # the effective corner energies leave the range of the eigenvalues by less than (1836 / 1260 - 1) / 2 of its width
        width = float(eig.max() - eig.min())
        lo, hi = float(eig.min()) - 0.25 * width, float(eig.max()) + 0.25 * width
        top = hi
        M = 512
        target = nstates * (1.0 - 1e-12)

        def narrow(a, b, states, reached):
            """the sub-interval (E_{i-1}, E_i] of M samples of [a, b] with `reached` first true at E_i -> (a', b', value at b', i)"""
            Es = a + (b - a) * (np.arange(M) / (M - 1.0))
            Es[-1] = b
            u = self.ltm_optimized(Es, states=states)
            hit = np.flatnonzero(reached(u[:-1]))
            i = int(hit[0]) if len(hit) else M - 1  # the upper end stands for "none": it was seen to qualify before
            return (float(Es[i - 1]) if i > 0 else a), float(Es[i]), float(u[i]), i

        Nhi = float(n)
        for _ in range(64):
            if not hi - lo > 0.0:
                break
            a, b, Nhi, i = narrow(lo, hi, True, lambda N: N >= target)
            shrunk = b - a < hi - lo
            lo, hi = a, b
            if i == 0 or hi - lo <= tol or not shrunk:
                break
        # below a gap N cannot tell the band top from a point 1e-4 below it, g can: the search of abz_rule_ltm_fermi on g == 0
        if top > hi:
            a, b, gap = hi, top, False
            for it in range(64):
                na, nb, g_at, i = narrow(a, b, False, lambda g: g == 0.0)
                if it == 0:
                    if g_at != 0.0 or i == 0:
                        break  # no zero of g above hi, or hi itself already has one
                    if self.ltm_optimized(np.array([nb]), states=True)[0] > nstates * (1.0 + 1e-12):
                        break  # states in between: the zero belongs to a higher gap
                    gap = True
                if i == 0:
                    b = a
                    break
                shrunk = nb - na < b - a
                a, b = na, nb
                if b - a <= tol or not shrunk:
                    break
            if gap:
                hi = b
                Nhi = float(self.ltm_optimized(np.array([hi]), states=True)[0])
        return hi, Nhi

    def ltm_green(self, zs, elements=None):
        """Trace of the Green's function tr G(z) = sum_b int dk / (z - e_b(k)) at the complex energies `zs`, per unit cell and
        summed over bands, as complex128 [nz] (abz_rule_ltm_green): the closed-form mean of 1 / (z - e) over every simplex of
        the mesh `ltm` scans, e linear inside a simplex.  -Im tr G(E + i eta) / pi is the DOS broadened by eta and tends to
        `ltm(E)` as eta -> 0; the error is the interpolation error O(1/npt^2) whatever eta is, where a grid sum of the
        resolvent needs npt >~ bandwidth / eta.  Every z needs Im z != 0 (Im z < 0 gives the conjugate of the value at conj z,
        to the bit); two calls return the same bits.  The rule must be a whole periodic grid (an unfolded rule is one); a
        k-sharded rule raises NotImplementedError, with or without its halo plane.

        `elements`: matrix elements A_b(k), linear inside a simplex like the energy; the result is then
        G_A(z) = sum_b int dk A_b(k) / (z - e_b(k)) as complex128 [nz, ncomp] (abz_rule_ltm_green_weighted), from the mean of
        lambda_i / (z - e) at every corner i of every simplex.  "energy": A = e itself (one component, z tr G(z) - n);
        "attached": what ltm_elements or ltm_orbitals attached (orbital weights give the diagonal G_aa(z) of the local
        Green's function); an array [ncomp, nk, n]: attached first."""
        self._ltm_refuse_shard("ltm_green")
        zs = np.ascontiguousarray(np.asarray(zs, dtype=np.complex128).reshape(-1))
        if elements is None:
            out = np.zeros(len(zs), dtype=np.complex128)
            h = self.h  # (a stale rule is refilled here)
            L.check(L.lib().abz_rule_ltm_green(h, zs.view(np.float64).ctypes.data_as(L.c_f64p), len(zs), out.view(np.float64).ctypes.data_as(L.c_f64p)))
            return out
        if isinstance(elements, str):
            if elements not in ("energy", "attached"):
                raise ValueError(f"ltm_green: elements = {elements!r} is neither 'energy' nor 'attached'")
        else:
            self.ltm_elements(elements)
            elements = "attached"
        h = self.h  # (a stale rule is refilled here, which drops the attached elements)
        ncomp = 1 if elements == "energy" else self._ltm_ncomp
        if ncomp < 1:
            raise ValueError("ltm_green: no matrix elements are attached (ltm_elements, ltm_orbitals; a rebuild of the rule drops them)")
        out = np.zeros((len(zs), ncomp), dtype=np.complex128)
        L.check(L.lib().abz_rule_ltm_green_weighted(h, L.LTM_A_ENERGY if elements == "energy" else L.LTM_A_ELEMENTS,
                                                    zs.view(np.float64).ctypes.data_as(L.c_f64p), len(zs),
                                                    out.view(np.float64).ctypes.data_as(L.c_f64p)))
        return out

    def ltm_green_optimized(self, zs, elements=None):
        """`ltm_green(zs, elements)` by the optimized tetrahedron method (abz_rule_ltm_green_optimized; d = 3): the closed-form
        means of 1 / (z - e) and lambda_i / (z - e) over every simplex, taken on the effective corner values e' and A' that
        `ltm_optimized` fits to 20 grid points per simplex.  -Im tr G(E + i eta) / pi tends to `ltm_optimized(E)` as eta -> 0,
        and the error at npt compares with that of `ltm_green` at 2 npt whatever eta is.  Same `elements` values and return
        shapes as `ltm_green`: None (tr G(z), complex128 [nz]), "energy" (z tr G(z) - n), "attached" or an array
        [ncomp, nk, n] ([nz, ncomp]).  Im z != 0; Im z < 0 gives the conjugate of the value at conj z, to the bit; two calls
        return the same bits.  This method and `dos.green_trace` / `dos.green_weighted` with `optimized=True` are the way to
        the optimized Green's functions: `LTM(optimized=True, eta=...)` is refused and the solve path with `eta` stays
        linear.  NotImplementedError on a k-sharded rule and for d < 3, before the library is asked."""
        self._ltm_refuse_optimized("ltm_green_optimized")
        zs = np.ascontiguousarray(np.asarray(zs, dtype=np.complex128).reshape(-1))
        if elements is None:
            source, ncomp = L.LTM_A_ONE, 1
        elif isinstance(elements, str):
            if elements not in ("energy", "attached"):
                raise ValueError(f"ltm_green_optimized: elements = {elements!r} is neither 'energy' nor 'attached'")
            source = L.LTM_A_ENERGY if elements == "energy" else L.LTM_A_ELEMENTS
        else:
            self.ltm_elements(elements)
            source = L.LTM_A_ELEMENTS
        h = self.h  # (a stale rule is refilled here, which drops the attached elements)
        if source == L.LTM_A_ELEMENTS:
            ncomp = self._ltm_ncomp
            if ncomp < 1:
                raise ValueError("ltm_green_optimized: no matrix elements are attached (ltm_elements, ltm_orbitals; a rebuild of the "
                                 "rule drops them)")
        elif source == L.LTM_A_ENERGY:
            ncomp = 1
        out = np.zeros((len(zs), ncomp), dtype=np.complex128)
        L.check(L.lib().abz_rule_ltm_green_optimized(h, source, zs.view(np.float64).ctypes.data_as(L.c_f64p), len(zs),
                                                     out.view(np.float64).ctypes.data_as(L.c_f64p)))
        return out[:, 0] if elements is None else out

    def ltm_node_weights(self, Es, states=True, correction=False, export=True):
        """Bloechl's integration weights w_b(k; E) per grid point and band (abz_rule_ltm_node_weights), [nE, nk, n] in the node
        and band order of export()'s eig: the numbers with N_A(E) = sum_k sum_b w_b(k; E) A_b(k) for ANY A (`states`, the
        default), g_A(E) likewise (`states=False`), or N_A with Bloechl's curvature correction (`correction=True`, validated
        as in `ltm`; the block then still sums to N(E)).  At most 16 energies per call, in any order.  The weights also stay
        on the device, tiled like attached elements, until the next call, a rebuild of the rule or `close`:
        `ltm_node_weights_dot` contracts them with attached elements without another walk over the simplices, and
        `export=False` (returns None) skips the copy to the host.  The rule must be a whole periodic grid (an unfolded rule
        is one); a k-sharded rule raises NotImplementedError, with or without its halo plane."""
        self._ltm_refuse_shard("ltm_node_weights")
        if correction and not states:
            raise ValueError("ltm_node_weights: correction=True corrects the state sum N_A: it needs states=True (the DOS has no correction)")
        Es = np.ascontiguousarray(np.asarray(Es, dtype=np.float64).reshape(-1))
        if not 1 <= len(Es) <= L.LTM_NODEW_MAX_E:
            raise ValueError(f"ltm_node_weights: {len(Es)} energies, a call takes 1..{L.LTM_NODEW_MAX_E}")
        what = L.LTM_STATES_CORRECTED if correction else (L.LTM_STATES if states else L.LTM_DOS)
        h = self.h  # (a stale rule is refilled here, which drops the weights it held)
        out = np.empty((len(Es), self.nk, self.nbands)) if export else None
        L.check(L.lib().abz_rule_ltm_node_weights(h, Es.ctypes.data_as(L.c_f64p), len(Es), what,
                                                  out.ctypes.data_as(L.c_f64p) if export else None))
        return out

    def ltm_node_weights_optimized(self, Es, states=True, export=True):
        """The integration weights w_b(k; E) of the optimized tetrahedron rule (abz_rule_ltm_node_weights_optimized; d = 3),
        [nE, nk, n] in the node and band order of export()'s eig: sum_k sum_b w A is the N_A(E) (`states`, the default) or
        g_A(E) (`states=False`) of `ltm_optimized` for ANY A; they sum to N(E) or g(E), and the occupations at
        `ltm_fermi_optimized`'s level sum to its state count.  Every simplex scatters the corner weights of the linear rule
        on its effective corner energies onto its 20 stencil points, so these weights are NOT confined to [0, 1 / nk]: a node
        next to the Fermi surface can weigh negative (nk w down to -0.12 has been seen).  There is no `correction`: this
        rule replaces it.  At most 16 energies per call, in any order.  The weights fill the same resident block as those of
        `ltm_node_weights`: `ltm_node_weights_ptr`, `ltm_node_weights_dot`, `ltm_node_weights_fold` and `ltm_density_matrix`
        (Es=None) work on them as they are; `export=False` (returns None) skips the copy to the host.  Two calls return the
        same bits, whatever ABZ_LTM_OPTW_CHUNK_MB (the scratch of a slab of grid planes) is.  The rule must be a whole
        periodic grid (an unfolded rule is one); NotImplementedError on a k-sharded rule and for d < 3."""
        self._ltm_refuse_optimized("ltm_node_weights_optimized")
        Es = np.ascontiguousarray(np.asarray(Es, dtype=np.float64).reshape(-1))
        if not 1 <= len(Es) <= L.LTM_NODEW_MAX_E:
            raise ValueError(f"ltm_node_weights_optimized: {len(Es)} energies, a call takes 1..{L.LTM_NODEW_MAX_E}")
        h = self.h  # (a stale rule is refilled here, which drops the weights it held)
        out = np.empty((len(Es), self.nk, self.nbands)) if export else None
        L.check(L.lib().abz_rule_ltm_node_weights_optimized(h, Es.ctypes.data_as(L.c_f64p), len(Es), L.LTM_STATES if states else L.LTM_DOS,
                                                            out.ctypes.data_as(L.c_f64p) if export else None))
        return out

    def ltm_node_weights_ptr(self):
        """(device address, bytes, nE) of the resident weight block of `ltm_node_weights`; (0, 0, 0) when there is none."""
        self._ltm_refuse_shard("ltm_node_weights_ptr")
        return self._ltm_ptr(L.lib().abz_rule_ltm_node_weights_ptr)

    def ltm_node_weights_dot(self, elements="attached"):
        """sum_k sum_b w_b(k; E_i) A_{c,b}(k) of the resident weights of `ltm_node_weights` as [nE, ncomp]
        (abz_rule_ltm_node_weights_dot): one pass over the two blocks, no walk over the simplices.  `elements`: "attached"
        (what ltm_elements, ltm_orbitals or ltm_projectors attached) or an array [ncomp, nk, n], attached first; attaching
        elements leaves the weights in place."""
        return self._node_weights_dot(False, elements)

    def _node_weights_dot(self, green, elements):
        """The resident real weights (float64 [nE, ncomp]) or, with `green`, complex ones (complex128 [nz, ncomp]) against the
        attached elements."""
        weights = "ltm_green_node_weights" if green else "ltm_node_weights"
        self._ltm_refuse_shard(f"{weights}_dot")
        if isinstance(elements, str):
            if elements != "attached":
                raise ValueError(f"{weights}_dot: elements = {elements!r} is neither 'attached' nor an array")
        else:
            self.h  # (a stale rule is refilled first: it loses its weights, and the call below says so)
            self.ltm_elements(elements)
        h = self.h
        _, _, count = getattr(self, f"{weights}_ptr")()
        if count < 1:
            raise ValueError(f"{weights}_dot: the rule holds no weights ({weights}; a rebuild of the rule drops them)")
        if self._ltm_ncomp < 1:
            raise ValueError(f"{weights}_dot: no matrix elements are attached (ltm_elements; a rebuild of the rule drops them)")
        out = np.zeros((count, self._ltm_ncomp), dtype=np.complex128 if green else np.float64)
        L.check(getattr(L.lib(), f"abz_rule_{weights}_dot")(h, out.view(np.float64).ctypes.data_as(L.c_f64p)))
        return out

    def ltm_density_matrix(self, Es=None, states=True, correction=False, orbitals=None, optimized=False):
        """The density matrix rho_pq(E) = sum_k sum_b w_b(k; E) U_pb(k) conj(U_qb(k)) in the orbital basis, per unit cell,
        complex128 [nE, m, m] (abz_rule_ltm_density_matrix): the resident weights of `ltm_node_weights` contracted with the
        eigenvectors inside one eigen-solve of the grid; U(k) and the band projectors never reach memory.  With `Es` the
        weights are made first (`ltm_node_weights(Es, states, correction, export=False)`, at most 16 energies); with
        `Es=None` the resident ones are used, and they say what rho is: the occupation matrix (`states`), the corrected one
        (`correction`) or the spectral-density matrix (`states=False`).  Hermitian to the bit; tr rho is N(E) or g(E); two
        calls return the same bits.  `orbitals` (None: all n) selects the sub-block rho[orbitals][:, orbitals] on the host.
        Nothing is attached: elements and weights stay as they were.  1...32 bands, a whole periodic grid with H(k) (not an
        unfolded rule); a k-sharded rule raises NotImplementedError.  `optimized=True` (d = 3, with `Es`): the weights are
        those of the optimized tetrahedron rule (`ltm_node_weights_optimized`), tr rho the N(E) or g(E) of `ltm_optimized`;
        it does not go with `correction`."""
        self._ltm_refuse_shard("ltm_density_matrix")
        if optimized and correction:
            raise ValueError("ltm_density_matrix: optimized=True replaces the curvature correction: it does not go with correction=True")
        if optimized and Es is None:
            raise ValueError("ltm_density_matrix: optimized=True makes the weights of Es (the resident ones are what the call that made "
                             "them says: give Es, or leave optimized out)")
        n = self.dev.s.n
        orb = density_matrix_orbitals(orbitals, n)
        if Es is not None and optimized:
            self.ltm_node_weights_optimized(Es, states=states, export=False)
        elif Es is not None:
            self.ltm_node_weights(Es, states=states, correction=correction, export=False)
        h = self.h  # (a stale rule is refilled here, which drops the weights it held)
        _, _, nE = self.ltm_node_weights_ptr()
        if nE < 1:
            raise ValueError("ltm_density_matrix: the rule holds no weights (give Es, or call ltm_node_weights; a rebuild of the "
                             "rule drops them)")
        out = np.zeros((nE, n, n), dtype=np.complex128)
        L.check(L.lib().abz_rule_ltm_density_matrix(h, out.view(np.float64).ctypes.data_as(L.c_f64p)))
        return out if orbitals is None else np.ascontiguousarray(out[:, orb][:, :, orb])

    def ltm_green_node_weights(self, zs, export=True):
        """The complex integration weights W_b(k; z) of the Green's function per grid point and band
        (abz_rule_ltm_green_node_weights), complex128 [nz, nk, n] in the node and band order of export()'s eig: the numbers
        with G_A(z) = sum_k sum_b W_b(k; z) A_b(k) for ANY A -- complex, matrix-valued, or not known yet -- where `ltm_green`
        takes real elements attached before its scan.  At most 8 values per call, Im z != 0, in any order; Im z < 0 gives the
        conjugate of the weights at conj z, to the bit; two calls return the same bits.  The weights also stay on the device in
        a block of their own (the real weights of `ltm_node_weights` are untouched) until the next call, a rebuild of the rule
        or `close`: `ltm_green_node_weights_dot` contracts them with attached elements, `ltm_green_node_weights_matrix` with
        the eigenvectors, and `export=False` (returns None) skips the copy to the host.  The rule must be a whole periodic grid
        (an unfolded rule is one); a k-sharded rule raises NotImplementedError, with or without its halo plane."""
        self._ltm_refuse_shard("ltm_green_node_weights")
        zs = green_node_weight_zs(zs)
        h = self.h  # (a stale rule is refilled here, which drops the weights it held)
        out = np.empty((len(zs), self.nk, self.nbands), dtype=np.complex128) if export else None
        L.check(L.lib().abz_rule_ltm_green_node_weights(h, zs.view(np.float64).ctypes.data_as(L.c_f64p), len(zs),
                                                        out.view(np.float64).ctypes.data_as(L.c_f64p) if export else None))
        return out

    def ltm_green_node_weights_optimized(self, zs, export=True):
        """The complex integration weights W_b(k; z) of the optimized tetrahedron rule (abz_rule_ltm_green_node_weights_optimized;
        d = 3), complex128 [nz, nk, n] in the node and band order of export()'s eig: sum_k sum_b W A is the G_A(z) of
        `ltm_green_optimized` for ANY A, sum W its tr G(z), sum W e = z tr G(z) - n.  Every simplex scatters the complex corner
        weights of the linear rule on its effective corner energies onto its 20 stencil points; the weights differ from those of
        `ltm_green_node_weights` by O(1 / npt^2).  At most 8 values per call, Im z != 0, in any order; Im z < 0 gives the
        conjugate of the weights at conj z, to the bit.  The weights fill the same resident block as those of
        `ltm_green_node_weights`: `ltm_green_node_weights_ptr`, `_dot`, `_fold` and `_matrix` (zs=None) work on them as they
        are, and the real weights of `ltm_node_weights` are untouched; `export=False` (returns None) skips the copy to the host.
        Two calls return the same bits, whatever ABZ_LTM_OPTW_CHUNK_MB (the scratch of a slab of grid planes) is.  The rule
        must be a whole periodic grid (an unfolded rule is one); NotImplementedError on a k-sharded rule and for d < 3."""
        self._ltm_refuse_optimized("ltm_green_node_weights_optimized")
        zs = green_node_weight_zs(zs, "ltm_green_node_weights_optimized")
        h = self.h  # (a stale rule is refilled here, which drops the weights it held)
        out = np.empty((len(zs), self.nk, self.nbands), dtype=np.complex128) if export else None
        L.check(L.lib().abz_rule_ltm_green_node_weights_optimized(h, zs.view(np.float64).ctypes.data_as(L.c_f64p), len(zs),
                                                                  out.view(np.float64).ctypes.data_as(L.c_f64p) if export else None))
        return out

    def ltm_green_node_weights_ptr(self):
        """(device address, bytes, nz) of the resident block of `ltm_green_node_weights`; (0, 0, 0) when there is none."""
        self._ltm_refuse_shard("ltm_green_node_weights_ptr")
        return self._ltm_ptr(L.lib().abz_rule_ltm_green_node_weights_ptr)

    def ltm_green_node_weights_dot(self, elements="attached"):
        """sum_k sum_b W_b(k; z_i) A_{c,b}(k) of the resident weights of `ltm_green_node_weights` as complex128 [nz, ncomp]
        (abz_rule_ltm_green_node_weights_dot): `ltm_green(zs, elements="attached")` without another walk over the simplices.
        `elements` as in `ltm_node_weights_dot`: "attached" or an array [ncomp, nk, n], attached first; attaching elements
        leaves the weights in place."""
        return self._node_weights_dot(True, elements)

    def ltm_green_node_weights_matrix(self, zs=None, orbitals=None, optimized=False):
        """The local Green's function G_pq(z) = sum_k sum_b W_b(k; z) U_pb(k) conj(U_qb(k)) in the orbital basis, per unit cell,
        complex128 [nz, m, m] (abz_rule_ltm_green_node_weights_matrix): the resident weights of `ltm_green_node_weights`
        contracted with the eigenvectors by the kernel of `ltm_density_matrix`; no projector is attached and attached elements
        stay as they were.  With `zs` (any number) the weights are made first, in chunks of 8; with `zs=None` the resident ones
        are used.  G(z)^dagger = G(conj z); two calls return the same bits.  `orbitals` (None: all n) selects the sub-block on
        the host.  Against `ltm_green_matrix`, which repeats the eigen-solve of the grid once per group of 16 projector
        components and scans the simplices per group: this route gathers the weights once per z and solves the grid once per 4
        weight sets for 1...4 bands, twice per z for 5...32 (`abz.dos.green_local` has the measured crossover: the number of
        projector groups).  1...32 bands, a whole periodic grid with H(k)
        (not an unfolded rule); a k-sharded rule raises NotImplementedError.  `optimized=True` (d = 3, with `zs`): the weights
        are those of the optimized tetrahedron rule (`ltm_green_node_weights_optimized`), tr G the tr G(z) of
        `ltm_green_optimized`."""
        self._ltm_refuse_shard("ltm_green_node_weights_matrix")
        if optimized and zs is None:
            raise ValueError("ltm_green_node_weights_matrix: optimized=True makes the weights of zs (the resident ones are what the "
                             "call that made them says: give zs, or leave optimized out)")
        if optimized:
            self._ltm_refuse_optimized("ltm_green_node_weights_matrix")
        n = self.dev.s.n
        orb = density_matrix_orbitals(orbitals, n, "ltm_green_node_weights_matrix")
        if zs is None:
            chunks = [None]
        else:
            zs = np.ascontiguousarray(np.asarray(zs, dtype=np.complex128).reshape(-1))
            step = L.LTM_GREEN_NODEW_MAX_Z
            chunks = [green_node_weight_zs(zs[i:i + step], "ltm_green_node_weights_matrix") for i in range(0, max(len(zs), 1), step)]
        parts = []
        for chunk in chunks:
            if chunk is not None and optimized:
                self.ltm_green_node_weights_optimized(chunk, export=False)
            elif chunk is not None:
                self.ltm_green_node_weights(chunk, export=False)
            h = self.h  # (a stale rule is refilled here, which drops the weights it held)
            _, _, nz = self.ltm_green_node_weights_ptr()
            if nz < 1:
                raise ValueError("ltm_green_node_weights_matrix: the rule holds no weights (give zs, or call ltm_green_node_weights; a "
                                 "rebuild of the rule drops them)")
            out = np.zeros((nz, n, n), dtype=np.complex128)
            L.check(L.lib().abz_rule_ltm_green_node_weights_matrix(h, out.view(np.float64).ctypes.data_as(L.c_f64p)))
            parts.append(out)
        G = parts[0] if len(parts) == 1 else np.concatenate(parts, axis=0)
        return G if orbitals is None else np.ascontiguousarray(G[:, orb][:, :, orb])

    def ltm_fermi(self, nstates, tol=1e-10):
        """(E_F, N(E_F)): the Fermi level of `nstates` states per unit cell, 0 < nstates < n, to within `tol`
        (abz_rule_ltm_fermi: a few N(E) scans of 512 energies each, no host bisection)."""
        self._ltm_refuse_shard("ltm_fermi (it needs an all-reduce inside the search)")
        ef, nf = C.c_double(0.0), C.c_double(0.0)
        L.check(L.lib().abz_rule_ltm_fermi(self.h, float(nstates), float(tol), C.byref(ef), C.byref(nf)))
        return ef.value, nf.value

    def ltm_pairs(self, lower, upper, operators=None, components=None):
        """The pair rule of two band ranges of this rule (abz_rule_ltm_pairs): a whole periodic grid whose "bands" are the
        differences e_c(k) - e_v(k), v in `lower`, c in `upper` (each a `range` or (start, count); lower below upper, at most 64
        pairs), pseudo-band (v - v0) nc + (c - c0).  Its `ltm(ws)` is the joint density of states.  With `operators` (1..4
        FourierSeries in the Wannier basis of H, or DeviceRules with H planes, as for `ltm_expectation`) it carries the
        interband products of M^i_vc = u_v^H Hermitian(O_i) u_c as attached elements: `components` entries i (|M^i|^2), (i, j)
        (Re M^i conj(M^j)) or (i, j, "re" | "im"); None: |M^i|^2 for every operator.  `ltm(ws, elements="attached")` is then the
        interband spectrum, `ltm_green(zs, elements="attached")` the broadened one (-Im / pi) with its Kramers-Kronig partner
        (Re).  At a degenerate level only the sum of a component over all pairs between two levels is defined.  These scans
        take whole bands; the occupation factors of a metal are `PairRule.ltm_occupied(ws, fermi)`."""
        self._ltm_refuse_shard("ltm_pairs")
        return PairRule(self, lower, upper, operators, components)

    def unfold(self):
        """The full-grid eigenvalue rule of this symmetric rule (abz_rule_ltm_unfold): every grid point gets the
        eigenvalues of the irreducible node in its orbit, e_b(S k) = e_b(k), by a gather on the device instead of npt^d
        eigensolves.  The symmetries must be symmetries of H (the contract GGR and PTR have on a symmetric zone).  The
        result serves `ltm`, `ltm_elements`, `ltm_fermi` and `export`, follows the series like any rule; while it is alive this
        rule hands out the same object."""
        self._ltm_refuse_shard("unfold")
        if self.syms is None:
            raise ValueError("unfold: the rule is a full grid already (no symmetries to unfold)")
        if not (self.want & L.WANT_EIG):
            raise ValueError("unfold: the rule holds no eigenvalues (want lacked WANT_EIG)")
        ref = getattr(self, "_unfolded", None)  # a weak reference: the unfolded rule holds this one, not the other way round
        u = ref() if ref is not None else None
        if u is None or u._closed:
            u = UnfoldedRule(self)
            self._unfolded = weakref.ref(u)
        return u


class UnfoldedRule(DeviceRule):
    """Whole periodic grid of eigenvalues gathered from the irreducible nodes of a symmetric DeviceRule
    (DeviceRule.unfold, abz_rule_ltm_unfold).  It holds eigenvalues only -- no H(k), no velocities -- and an orbit map of
    4 B per grid point; `ltm`, `ltm_elements`, `ltm_fermi`, `export(eig=True)`, `npt`, `nk = npt^d` and `close` are those
    of a full-grid rule."""

    def __init__(self, source: DeviceRule):
        dev = self.dev = source.dev
        d, n = dev.s.d, dev.s.n
        self.source = source
        self.npt = source.npt
        self.want = L.WANT_EIG
        self.syms = None  # a full grid to every reader
        self.nsyms = 1
        self.shard = None
        self.nk = self.nk_local = self.npt ** d
        self._S = np.ascontiguousarray(np.rint(np.asarray(source.syms)).astype(np.int32).reshape(-1, d, d))
        self._hbox = C.c_void_p()
        src = source.h  # (a stale source is refilled here)
        L.check(L.lib().abz_rule_ltm_unfold(src, self._S.ctypes.data_as(L.c_i32p), len(self._S), C.byref(self._hbox)))
        self._adopt(self._hbox)
        self.nbytes = (8 * n + 4) * self.nk

    def _source(self):
        if self.source._closed:  # the series' rule cache let it go: the same nodes again
            self.source = self.dev.rule(self.npt, self.source.syms, self.source.want)
        return self.source

    def _gather(self):
        self._source()
        self.generation = self.dev.generation
        self._ltm_ncomp = 0  # the library drops attached matrix elements with the old eigenstates
        L.check(L.lib().abz_rule_ltm_unfold(self.source.h, self._S.ctypes.data_as(L.c_i32p), len(self._S), C.byref(self._hbox)))

    @property
    def h(self):
        """The abz_rule handle; when the series moved on, the source is refilled and the planes are gathered again."""
        if self._closed:
            raise L.AbzError("DeviceRule was closed")
        if self.generation != self.dev.generation:
            self._gather()
        return self._h

    def rebuild(self):
        if self._closed:
            raise L.AbzError("DeviceRule was closed")
        self._source().rebuild()
        self._gather()

    def unfold(self):
        raise ValueError("unfold: the rule is a full grid already (no symmetries to unfold)")

    def ltm_node_weights_fold(self):
        """The resident weights of `ltm_node_weights` summed over each orbit onto the irreducible nodes of the source rule,
        [nE, nirr, n] in the source's node order (abz_rule_ltm_node_weights_fold): sum_j sum_b fold_b(j) A_b(j) is then the
        full-grid N_A of any A that the zone's symmetries leave alone, from values at the irreducible nodes only.  The Kuhn
        mesh is invariant under 12 of the 48 cubic operations, so this is a sum over the orbit, not multiplicity x weight."""
        h = self.h
        _, _, nE = self.ltm_node_weights_ptr()
        if nE < 1:
            raise ValueError("ltm_node_weights_fold: the rule holds no weights (ltm_node_weights; a new gather drops them)")
        out = np.zeros((nE, len(self.source), self.dev.s.n))
        L.check(L.lib().abz_rule_ltm_node_weights_fold(h, out.ctypes.data_as(L.c_f64p)))
        return out

    def ltm_green_node_weights_fold(self):
        """The resident weights of `ltm_green_node_weights` summed over each orbit onto the irreducible nodes of the source
        rule, complex128 [nz, nirr, n] in the source's node order (abz_rule_ltm_green_node_weights_fold):
        sum_j sum_b fold_b(j) A_b(j) is then the full-grid G_A(z) of any A that the zone's symmetries leave alone, from values
        at the irreducible nodes only.  A sum over the orbit, not multiplicity x weight (`ltm_node_weights_fold`)."""
        h = self.h
        _, _, nz = self.ltm_green_node_weights_ptr()
        if nz < 1:
            raise ValueError("ltm_green_node_weights_fold: the rule holds no weights (ltm_green_node_weights; a new gather drops them)")
        out = np.zeros((nz, len(self.source), self.dev.s.n), dtype=np.complex128)
        L.check(L.lib().abz_rule_ltm_green_node_weights_fold(h, out.view(np.float64).ctypes.data_as(L.c_f64p)))
        return out


class PairRule(DeviceRule):
    """Whole periodic grid of band-pair energies e_c(k) - e_v(k) with, optionally, interband products as attached elements
    (DeviceRule.ltm_pairs, abz_rule_ltm_pairs).  `nbands` = nv nc pseudo-bands, `lower` / `upper` the ranges; `ltm`,
    `ltm_green`, `ltm_elements`, `ltm_elements_export`, `ltm_node_weights`, `ltm_green_node_weights` with their dots, `ltm_fermi`
    and `export(x, w, eig)` are those of a full-grid rule of nbands bands.  It holds no H(k), no eigenvectors and no plan: what
    needs them (`ltm_orbitals`, `ltm_projectors`, `ltm_expectation`, `ltm_density_matrix`, `ltm_green_matrix`, `reduce`, a pair rule
    of it) raises with the library's message.  It follows the series: when the coefficients changed, the source is refilled
    and `refill` repeats the call into the same handle."""

    def __init__(self, source: DeviceRule, lower, upper, operators=None, components=None):
        dev = self.dev = source.dev
        d = dev.s.d
        self.source = source
        self.npt = source.npt
        self.want = L.WANT_EIG
        self.syms = None  # a full grid to every reader
        self.nsyms = 1
        self.shard = None
        self.nk = self.nk_local = self.npt ** d
        v0, nv, c0, nc = pair_ranges(lower, upper, dev.s.n if not isinstance(source, PairRule) else None)
        self.lower, self.upper = range(v0, v0 + nv), range(c0, c0 + nc)
        ops = [] if operators is None else (list(operators) if isinstance(operators, (list, tuple)) else [operators])
        if operators is not None and not 1 <= len(ops) <= L.LTM_PAIRS_MAX_OPS:
            raise ValueError(f"ltm_pairs: {len(ops)} operators, a call takes 1..{L.LTM_PAIRS_MAX_OPS}")
        if not ops and components is not None:
            raise ValueError("ltm_pairs: components without operators")
        self.operators = ops
        self._comps = pair_components(components, len(ops)) if ops else None
        self._hbox = C.c_void_p()
        self._fill()
        self._adopt(self._hbox)
        self._ltm_ncomp = self._ncomp
        self.nbytes = 8 * nv * nc * (1 + self._ncomp) * self.nk

    @property
    def _ncomp(self):
        return 0 if not self.operators else (len(self.operators) if self._comps is None else len(self._comps))

    def _fill(self):
        src = self.source.h  # (a stale source is refilled here)
        rules = self.source._operator_rules(self.operators, "ltm_pairs")
        handles = (C.c_void_p * max(len(rules), 1))(*[getattr(r.h, "value", None) for r in rules])  # (stale operator rules are refilled here)
        comps = self._comps
        L.check(L.lib().abz_rule_ltm_pairs(src, self.lower.start, len(self.lower), self.upper.start, len(self.upper),
                                           handles if rules else None, len(rules), None if comps is None else comps.ctypes.data_as(L.c_i32p),
                                           self._ncomp, C.byref(self._hbox)))

    def refill(self, source=None):
        """Energies and elements again from `source` (default: the rule this one was made from) into the same handle: the call
        to make after the series changed.  Weight blocks are dropped, elements attached by hand are replaced by the rule's own."""
        if self._closed:
            raise L.AbzError("DeviceRule was closed")
        if source is not None:
            self.source = source
        elif self.source._closed:  # the series' rule cache let it go: the same grid again
            self.source = self.dev.rule(self.npt, self.source.syms, self.source.want)
        self.generation = self.dev.generation
        self._fill()
        self._ltm_ncomp = self._ncomp

    @property
    def h(self):
        """The abz_rule handle; when the series moved on, the source is refilled and the pair rule filled again."""
        if self._closed:
            raise L.AbzError("DeviceRule was closed")
        if self.generation != self.dev.generation:
            self.refill()
        return self._h

    def rebuild(self):
        if self._closed:
            raise L.AbzError("DeviceRule was closed")
        self.source.rebuild()
        self.refill()

    def ltm_occupied(self, ws, fermi, states=False, elements=None):
        """The scans of this pair rule with the T = 0 occupations of a metal (abz_rule_ltm_pairs_occupied): the factor
        theta(fermi - e_v) theta(e_c - fermi) restricts every simplex to its occupied part -- the simplex cut by two planes, since
        e_v, e_c and e_c - e_v are all linear inside it -- which is split into sub-simplices that go through the closed forms of
        `ltm`.  `elements` None: the occupied joint density of states J^occ(w) as [nw]; "attached": the occupied interband spectra
        S^occ_ij(w) of the attached products as [nw, ncomp].  `states`: the cumulative forms (theta(w - Delta) for delta).  The band
        energies are read from `self.source` (refilled like `h` when the series moved on); a corner is occupied iff e_v <= fermi and
        empty iff e_c > fermi, the half-open rule of the scans.  `fermi` is the caller's: `self.source.ltm_fermi(nstates)` gives
        the grid's own level.  No curvature correction, no finite temperature, no broadened form."""
        if elements is not None and not (isinstance(elements, str) and elements == "attached"):
            raise ValueError(f"ltm_occupied: elements = {elements!r} is neither None nor 'attached'")
        fermi = float(fermi)
        if not np.isfinite(fermi):
            raise ValueError(f"ltm_occupied: fermi = {fermi!r} is not finite")
        ws = np.ascontiguousarray(np.asarray(ws, dtype=np.float64).reshape(-1))
        if len(ws) < 1:
            raise ValueError("ltm_occupied: no transition energies")
        if not self._closed and self.source._closed:  # the series' rule cache let the source go: the same grid again
            self.refill()
        h = self.h  # (a stale rule is refilled here, and its source with it)
        src = self.source.h
        if elements is None:
            out = np.zeros(len(ws))
            source = L.LTM_A_ONE
        else:
            if self._ltm_ncomp < 1:
                raise ValueError("ltm_occupied: the pair rule has no elements (ltm_pairs with operators, ltm_elements)")
            out = np.zeros((len(ws), self._ltm_ncomp))
            source = L.LTM_A_ELEMENTS
        L.check(L.lib().abz_rule_ltm_pairs_occupied(src, h, fermi, source, ws.ctypes.data_as(L.c_f64p), len(ws),
                                                    L.LTM_STATES if states else L.LTM_DOS, out.ctypes.data_as(L.c_f64p)))
        return out

    def unfold(self):
        raise ValueError("unfold: the rule is a full grid already (no symmetries to unfold)")

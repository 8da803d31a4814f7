"""Integration weights per grid point and band on the device (abz_rule_ltm_node_weights, _ptr, _dot, _fold; ltm_nodew_kernel,
ltm_nodew_dot_kernel and ltm_nodew_fold_kernel of kernels_ltm_nodew.hip) against the scatter-form restatement of
tests/nodew_numpy.py, against the shipped scans, and their exact values, repeatability, lifetime and refusals.

Parity bound: the restatement is fed the rule's own exported eigenvalues, so only summation order and FMA contraction remain.  A
node weight is a sum of at most 24 terms of exactly the kind the scans sum, of size 1 / nk: the project's LTM parity bound
(test_gpu_ltm.py) applied to the O(1) quantity nk w,   |nk u - nk ref| <= 1e-9 max(1, max|nk ref|).

Shapes: the smallest at which the gather can go wrong -- npt = 2 (k + 1 and k - 1 are the same node), 3, odd sizes, a 1-D line
longer than a wave (65, row padded to 80), 2 and 3 variables, one and several bands, 6 and 33 bands (blockIdx.y beyond one kernel
family of the eigenvalue builds)."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import abz_oracle as orc
import ltm_numpy as ln
import nodew_numpy as nw
import unfold_numpy as un
import test_gpu_mem_books as mb
from test_gpu_ltm import GOLD, product_series
from test_ltm_cpu import MODELS
from test_ltm_unfold_cpu import model_sym_sets

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def two_band_chain(abz):
    """A 1-D two-band model (a dimerised chain with an on-site splitting and a second-neighbour term)"""
    c = np.zeros((3, 2, 2), dtype=np.complex128)
    c[1] = [[0.3, 1.0], [1.0, -0.3]]
    c[2] = [[0.1, 0.5], [0.0, -0.15]]
    c[0] = c[2].conj().T
    return abz.FourierSeries(c, period=1.0, first=(-1,), ndim=1)


def flat_band_series(abz):
    """diag(e(k), e(k), 0.25) of test_ltm_flat_and_degenerate_bands_on_device"""
    so = orc.tb_integer(3)
    c = np.zeros((3, 3, 3, 3, 3), dtype=np.complex128)
    c[..., 0, 0] = so.c[..., 0, 0]
    c[..., 1, 1] = so.c[..., 0, 0]
    c[1, 1, 1, 2, 2] = 0.25
    return abz.FourierSeries(c, period=1.0, first=(-1, -1, -1), ndim=3)


def series_of(abz, name):
    if name in MODELS:
        return product_series(abz, MODELS[name][0]())
    if name == "chain2":
        return two_band_chain(abz)
    if name == "svo":
        return abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    return product_series(abz, orc.synthetic_wannier(int(name[3:]), rmax=2, seed=7))


CASES = [("int1", 2), ("int1", 3), ("int1", 65), ("chain2", 2), ("chain2", 3), ("chain2", 65),
         ("int2", 2), ("int2", 5), ("int2", 17), ("graphene", 2), ("graphene", 5), ("graphene", 17),
         ("int3", 2), ("int3", 3), ("int3", 5), ("svo", 6), ("syn6", 5), ("syn33", 5)]


def energy_list(eig, rng):
    """16 energies: below and above all bands, the exact band minimum and maximum, the eigenvalue of a node, the Gamma
    eigenvalues, random ones inside the bands in no order, one of them twice."""
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo if hi > lo else 1.0
    gamma = eig[(0,) * (eig.ndim - 1)]
    flat = eig.reshape(-1)
    inside = lo + w * rng.random(8)
    return np.concatenate([[lo - 0.3 * w, hi + 0.3 * w, lo, hi, flat[(7 * len(flat)) // 11], gamma[0], gamma[-1]], inside, inside[:1]])


# the calls of 1, 5 and 16 energies (a group of 4 and a remainder; 16: four groups): positions in energy_list
CALLS = {1: [8], 5: [9, 1, 4, 0, 9], 16: list(range(16))}
KIND_ARGS = {"dos": dict(states=False), "states": dict(states=True), "corrected": dict(states=True, correction=True)}


def close_nk(u, ref, nk):
    """(deviation, bound) of the parity check on nk w"""
    return float(np.abs(nk * np.asarray(u) - nk * np.asarray(ref)).max()), 1e-9 * max(1.0, float(np.abs(nk * np.asarray(ref)).max()))


def check_nk(u, ref, nk, what):
    assert u.shape == ref.shape and np.all(np.isfinite(u)), (what, u.shape, ref.shape)
    dev, bound = close_nk(u, ref, nk)
    print(f"nodew {what}: max dev of nk w {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)
    return dev / bound


def check(u, ref, what):
    u, ref = np.asarray(u), np.asarray(ref)
    assert u.shape == ref.shape and np.all(np.isfinite(u)), (what, u.shape, ref.shape)
    dev, bound = float(np.abs(u - ref).max()), 1e-9 * max(1.0, float(np.abs(ref).max()))
    print(f"nodew {what}: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)


def on_nodes(rule, Wgrid):
    """restatement weights [nE] + [npt]*d + [n] -> [nE, nk, n], the order of the export"""
    return Wgrid.reshape(Wgrid.shape[0], rule.nk, Wgrid.shape[-1])


def read_block(abz, rule):
    """The resident weight block through ltm_node_weights_ptr and hipMemcpy: [ntiles, nE n planes, row]"""
    L = abz._lib
    base, nbytes, nE = rule.ltm_node_weights_ptr()
    assert base and nbytes > 0 and nE > 0
    n, d, npt = rule.dev.s.n, rule.dev.s.d, rule.npt
    row = (npt + 15) // 16 * 16
    assert nbytes == 8 * npt ** (d - 1) * nE * n * row
    buf = np.empty(nbytes // 8)
    memcpy = L.lib().hipMemcpy  # (the HIP runtime the library is linked against)
    memcpy.restype, memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert memcpy(buf.ctypes.data, base, nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return buf.reshape(npt ** (d - 1), nE * n, row)


# ---------------------------------------------------------------- 1. parity with the restatement
@pytest.mark.parametrize("name,npt", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_node_weights_match_restatement(abz, name, npt):
    s = series_of(abz, name)
    rule = s.device().rule(npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    n = eig.shape[-1]
    Es = energy_list(eig, np.random.default_rng(5))
    simp = nw.simplices(eig)
    worst = 0.0
    for kind, kw in KIND_ARGS.items():
        ref = on_nodes(rule, nw.node_weights_from(simp, eig.shape, Es, kind))  # once per kind, for the calls of 1, 5 and 16
        for nE, pick in CALLS.items():
            W = rule.ltm_node_weights(Es[pick], **kw)
            assert W.shape == (nE, rule.nk, n)
            worst = max(worst, check_nk(W, ref[pick], rule.nk, f"{name} npt={npt} {kind} nE={nE}"))
            assert rule.ltm_node_weights_ptr()[2] == nE
    print(f"nodew parity {name} npt={npt}: worst deviation / bound = {worst:.3e}")


def test_node_weights_flat_and_degenerate_bands(abz):
    """diag(e, e, 0.25): two exactly degenerate bands and a flat one crossing them.  N (plain and corrected) at every energy,
    0.25 and its neighbours included; g away from 0.25 +- ulp, as in test_gpu_ltm_weighted.py."""
    rule = flat_band_series(abz).device().rule(4, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    Es = np.array([-7.0, -1.0, np.nextafter(0.25, -1.0), 0.25, np.nextafter(0.25, 1.0), 0.3, 2.0, 7.0])
    away = np.array([0, 1, 5, 6, 7])
    simp = nw.simplices(eig)
    for kind, kw in KIND_ARGS.items():
        E = Es[away] if kind == "dos" else Es
        ref = on_nodes(rule, nw.node_weights_from(simp, eig.shape, E, kind))
        check_nk(rule.ltm_node_weights(E, **kw), ref, rule.nk, f"degenerate {kind}")


# ---------------------------------------------------------------- 2. against the shipped scans
@pytest.mark.parametrize("name,npt", [("chain2", 65), ("int2", 17), ("svo", 6), ("syn6", 5)])
def test_node_weights_against_the_shipped_scans(abz, name, npt):
    s = series_of(abz, name)
    rule = s.device().rule(npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    n = eig.shape[-1]
    Es = energy_list(eig, np.random.default_rng(9))
    A = np.random.default_rng(2).standard_normal((16, rule.nk, n))
    rule.ltm_elements(A)
    for kind, kw in KIND_ARGS.items():
        scan = rule.ltm(Es, elements="attached", **kw)  # [16, 16]
        for nE, pick in CALLS.items():
            W = rule.ltm_node_weights(Es[pick], **kw)
            check(np.einsum("ekb,ckb->ec", W, A), scan[pick], f"{name} {kind} nE={nE} einsum(W, A) against the scan")
            dot = rule.ltm_node_weights_dot()
            assert dot.shape == (nE, 16)
            check(dot, scan[pick], f"{name} {kind} nE={nE} dot against the scan")
            if kind != "corrected":
                check(W.sum(axis=(1, 2)), rule.ltm(Es[pick], states=kw["states"]), f"{name} {kind} nE={nE} sum of the weights")
    # an array attaches first and leaves the weights in place; fewer components than 16
    few = rule.ltm_node_weights_dot(A[:3])
    check(few, rule.ltm(Es, states=True, elements="attached", correction=True), f"{name} dot of 3 components")
    rule.ltm_elements(None)
    assert rule.ltm_node_weights_ptr()[2] == 16  # dropping ELEMENTS leaves the weights alone


# ---------------------------------------------------------------- 3. exact values
@pytest.mark.parametrize("name,npt", [("int1", 2), ("chain2", 65), ("graphene", 5), ("int3", 3), ("svo", 6)])
def test_node_weights_exact_values(abz, name, npt):
    s = series_of(abz, name)
    rule = s.device().rule(npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    n, nk = eig.shape[-1], rule.nk
    lo, hi = float(eig.min()), float(eig.max())
    inside = float(np.sort(eig.reshape(-1))[eig.size // 3])  # (the middle of lo and hi may lie in a gap)
    Es = np.array([lo - 1.0, hi + 1.0, np.nextafter(lo, -np.inf), hi, inside])
    S = rule.ltm_node_weights(Es, states=True)
    Cw = rule.ltm_node_weights(Es, states=True, correction=True)
    G = rule.ltm_node_weights(Es, states=False)
    for W in (S, Cw, G):
        assert np.all(W[0] == 0.0) and np.all(W[2] == 0.0)  # exactly nothing below the bands
    assert np.all(G[1] == 0.0) and np.all(G[3] == 0.0)
    for W in (S, Cw):
        for i in (1, 3):  # every simplex lies wholly below: 1 / nk, an integer count divided once
            dev = float(np.abs(nk * W[i] - 1.0).max())
            print(f"{name} npt={npt}: max |nk w - 1| above the bands = {dev:.2e} ({dev / EPS:.1f} eps)")
            assert dev <= 4 * EPS
    # the correction sums to zero (kappa_T = 0 for A = 1): every weight is a sum of at most 24 terms of a few eps / nk each, so
    # the nk n differences sum to at most ~100 n eps; 1e-12 n leaves room
    tot = np.abs((Cw - S).sum(axis=(1, 2)))
    print(f"{name} npt={npt}: |sum of the correction| = {tot.max():.2e}, its largest entry nk |dw| = {nk * np.abs(Cw - S).max():.2e}")
    assert tot.max() <= 1e-12 * n
    if hi > lo:
        assert np.abs(Cw[4] - S[4]).max() > 0.0


# ---------------------------------------------------------------- 4. repeatability, padding
@pytest.mark.parametrize("name,npt", [("chain2", 65), ("int2", 5), ("svo", 6)])
def test_node_weights_repeatable_and_padding_is_zero(abz, name, npt):
    s = series_of(abz, name)
    rule = s.device().rule(npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    n, d = eig.shape[-1], rule.dev.s.d
    Es = energy_list(eig, np.random.default_rng(3))
    rule.ltm_elements(np.random.default_rng(4).standard_normal((5, rule.nk, n)))
    for kw in KIND_ARGS.values():
        for pick in CALLS.values():
            a = rule.ltm_node_weights(Es[pick], **kw)
            da = rule.ltm_node_weights_dot()
            block_a = read_block(abz, rule)
            b = rule.ltm_node_weights(Es[pick], **kw)
            db = rule.ltm_node_weights_dot()
            block = read_block(abz, rule)
            assert np.array_equal(a, b) and np.array_equal(da, db) and np.array_equal(block_a, block)
            assert np.all(block[:, :, npt:] == 0.0)  # the padding columns
            assert not np.any(np.signbit(block[:, :, npt:]))
            # the block is the export: plane i n + b of line l, column c = w_b(k = l npt + c; E_i)
            got = block[:, :, :npt].reshape(npt ** (d - 1), len(pick), n, npt).transpose(1, 0, 3, 2).reshape(len(pick), rule.nk, n)
            assert np.array_equal(got, b)
    assert rule.ltm_node_weights(Es[:5], export=False) is None and rule.ltm_node_weights_ptr()[2] == 5
    rule.ltm_elements(None)


# ---------------------------------------------------------------- 5. unfolded rules
@pytest.mark.parametrize("name,npt", [("int3", 4), ("int3", 6), ("svo", 4), ("svo", 6)])
def test_node_weights_of_an_unfolded_rule_and_their_fold(abz, name, npt):
    L = abz._lib
    s = series_of(abz, name)
    dev = s.device()
    syms = model_sym_sets(abz, name, 3)["cubic"]
    src = abz.DeviceRule(dev, npt, syms, L.WANT_EIG)
    unf = src.unfold()
    full = dev.rule(npt, None, L.WANT_EIG)
    eig = ln.rule_eigenvalues(unf)
    n, nk, nirr = eig.shape[-1], unf.nk, src.nk
    lo, hi = float(eig.min()), float(eig.max())
    Es = np.concatenate([[lo - 0.1, hi + 0.1], lo + (hi - lo) * np.random.default_rng(6).random(5)])
    se = src.export(eig=True)
    node_of = un.orbit_map(npt, 3, syms, se["x"])  # the orbits on the host, from the exported nodes and the matrices
    simp = nw.simplices(eig)
    for kind, kw in KIND_ARGS.items():
        W = unf.ltm_node_weights(Es, **kw)
        check_nk(W, full.ltm_node_weights(Es, **kw), nk, f"{name} npt={npt} {kind} unfolded against the full build")
        ref = on_nodes(unf, nw.node_weights_from(simp, eig.shape, Es, kind))
        check_nk(W, ref, nk, f"{name} npt={npt} {kind} unfolded against the restatement")
        fold = unf.ltm_node_weights_fold()
        assert fold.shape == (len(Es), nirr, n)
        fold_ref = np.zeros_like(fold)
        np.add.at(fold_ref, (slice(None), node_of), ref)
        # an orbit holds at most 48 points: the bound on nk w, for sums of up to 48 of them
        check_nk(fold, fold_ref, nk, f"{name} npt={npt} {kind} fold against the restatement's orbit sums")
        check(fold.sum(axis=(1, 2)), W.sum(axis=(1, 2)), f"{name} npt={npt} {kind} fold.sum against W.sum")
        assert np.array_equal(fold, unf.ltm_node_weights_fold())  # no atomics: the same bits
        if kind != "dos":  # the mesh has 12 of the 48 operations: a fold is not multiplicity x weight
            rep = np.array([np.flatnonzero(node_of == j)[0] for j in range(nirr)])
            assert np.abs(fold[2:] - se["w"][None, :, None] * W[2:, rep]).max() * nk > 1e-3
        # A = f(e) is exactly symmetric (unfolded eigenvalues are copies): folded sum on the irreducible nodes = full-grid scan
        for f in (np.square, np.sin):
            A = f(unf.export(x=False, w=False, eig=True)["eig"])[None]
            scan = unf.ltm(Es, elements=A, **kw)[:, 0]
            check(np.einsum("ejb,jb->e", fold, f(se["eig"])), scan, f"{name} npt={npt} {kind} folded sum of {f.__name__}(e)")
        unf.ltm_elements(None)


# ---------------------------------------------------------------- 6. lifetime
def test_node_weights_follow_the_rule(abz):
    """Dropped by a rebuild and by an update of the series (the old eigenvalues are gone), replaced by the next call."""
    s = two_band_chain(abz)
    rule = s.device().rule(9, None, abz._lib.WANT_EIG)
    Es = np.array([0.1, 0.4, -0.2])
    rule.ltm_node_weights(Es)
    assert rule.ltm_node_weights_ptr()[1:] == (8 * 3 * 2 * 16, 3)
    rule.ltm_node_weights(Es[:1], states=False)
    assert rule.ltm_node_weights_ptr()[1:] == (8 * 1 * 2 * 16, 1)
    rule.rebuild()
    assert rule.ltm_node_weights_ptr() == (0, 0, 0)
    with pytest.raises(ValueError, match="holds no weights"):
        rule.ltm_node_weights_dot(np.ones((1, 9, 2)))
    W1 = rule.ltm_node_weights(Es)
    s.c *= 1.5
    s.invalidate()
    assert rule.ltm_node_weights_ptr() == (0, 0, 0)
    W2 = rule.ltm_node_weights(1.5 * Es)
    check_nk(W2, W1, 9, "weights of the scaled series at the scaled energies")


def test_node_weights_are_accounted(abz):
    """abz_mem_info counts the block and the fold's inverse map; destroying the rules and the series gives everything back
    (the pattern of test_gpu_mem_books.py, on the C ABI)."""
    L = abz._lib
    lib = L.lib()
    gc.collect()
    gc.disable()
    try:
        for attempt in range(2):  # the first round warms the allocator's pool: blocks, not bytes, could differ
            b0 = mb.books(L, None)
            ctx = mb.create_ctx(L)
            s = mb.create_series(L, ctx, 2, seed=6)
            full = mb.build_full(L, s, L.WANT_EIG)
            src = mb.build_sym(L, s, L.WANT_EIG)
            unf = C.c_void_p()
            L.check(mb.unfold(L, src, mb.SYMS, unf))
            Es = np.array([0.1, -0.3, 0.2, 0.0, 0.5])
            pE = Es.ctypes.data_as(L.c_f64p)
            b1 = mb.books(L, ctx)
            L.check(lib.abz_rule_ltm_node_weights(full, pE, 5, L.LTM_STATES, None))
            b2 = mb.books(L, ctx)
            block = 8 * mb.NPT * 5 * 2 * 16  # lines x energies x bands x padded row
            assert b2[0] - b1[0] >= block and b2[1] == b1[1] + 1
            L.check(lib.abz_rule_ltm_node_weights(full, pE, 5, L.LTM_DOS, None))  # replaced, not added
            b2b = mb.books(L, ctx)  # (the allocator may hand out a cached block with more room: blocks are counted as they come)
            assert b2b[1] == b2[1] and block <= b2b[0] - b1[0] <= 2 * block
            nirr = C.c_int64(0)
            L.check(lib.abz_rule_info(src, C.byref(nirr), None, None, None, None))
            fold = np.zeros((5, max(nirr.value, mb.NPT ** 2), 2))
            # (with the export: the context's staging block, which the fold uses too, exists from here on)
            L.check(lib.abz_rule_ltm_node_weights(unf, pE, 5, L.LTM_STATES, fold.ctypes.data_as(L.c_f64p)))
            b3 = mb.books(L, ctx)
            L.check(lib.abz_rule_ltm_node_weights_fold(unf, fold.ctypes.data_as(L.c_f64p)))
            b4 = mb.books(L, ctx)
            assert b4[1] == b3[1] + 1 and b4[0] - b3[0] >= 8 * (nirr.value + 1) + 4 * mb.NPT ** 2  # the inverse map, kept
            L.check(lib.abz_rule_ltm_node_weights_fold(unf, fold.ctypes.data_as(L.c_f64p)))
            assert mb.books(L, ctx) == b4
            L.check(lib.abz_rule_rebuild(full))  # drops the block
            assert mb.books(L, ctx)[1] == b4[1] - 1
            L.check(lib.abz_rule_ltm_node_weights(full, pE, 5, L.LTM_STATES, None))
            mb.destroy(L, full, unf, src)  # with the weights resident
            assert lib.abz_series_destroy(s) == 0
            assert lib.abz_ctx_destroy(ctx) == 0
            b5 = mb.books(L, None)
            print(f"books (live bytes, live blocks): start {b0}, rules {b1}, weights {b2}, unfolded weights {b3}, fold {b4}, end {b5}")
            if attempt == 1:
                assert b5 == b0
    finally:
        gc.enable()


# ---------------------------------------------------------------- 7. refusals
def test_node_weight_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    npt = 4
    Es = np.array([0.5, 1.5, -0.5])
    pE = Es.ctypes.data_as(L.c_f64p)
    out = np.full(16 * npt ** 3, -99.0)
    pout = out.ctypes.data_as(L.c_f64p)
    full = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    h = full._h
    kept = full.ltm_node_weights(Es)
    kept_ptr = full.ltm_node_weights_ptr()
    kept_block = read_block(abz, full)

    def refused(rc, code, match=None):
        msg = lib.abz_last_error().decode()
        assert rc == code and len(msg) > 0, (rc, code, msg)
        assert match is None or match in msg, msg
        assert np.all(out == -99.0)  # nothing was written
        # the block computed before is where it was, readable and unchanged
        assert full.ltm_node_weights_ptr() == kept_ptr and np.array_equal(read_block(abz, full), kept_block)

    bad = np.array([0.5, np.nan, np.inf])
    refused(lib.abz_rule_ltm_node_weights(h, pE, 0, L.LTM_STATES, pout), L.ERR_ARG, "outside 1..16")
    refused(lib.abz_rule_ltm_node_weights(h, pE, 17, L.LTM_STATES, pout), L.ERR_ARG, "outside 1..16")
    refused(lib.abz_rule_ltm_node_weights(h, pE, -1, L.LTM_STATES, pout), L.ERR_ARG)
    refused(lib.abz_rule_ltm_node_weights(h, bad.ctypes.data_as(L.c_f64p), 2, L.LTM_STATES, pout), L.ERR_ARG, "not finite")
    refused(lib.abz_rule_ltm_node_weights(h, bad[[0, 2]].copy().ctypes.data_as(L.c_f64p), 2, L.LTM_STATES, pout), L.ERR_ARG, "not finite")
    refused(lib.abz_rule_ltm_node_weights(h, None, 3, L.LTM_STATES, pout), L.ERR_ARG)
    for what in (3, -1, 7):
        refused(lib.abz_rule_ltm_node_weights(h, pE, 3, what, pout), L.ERR_ARG, "what")
    refused(lib.abz_rule_ltm_node_weights_dot(h, pout), L.ERR_ARG, "no matrix elements")  # weights, nothing attached
    refused(lib.abz_rule_ltm_node_weights_dot(h, None), L.ERR_ARG)
    refused(lib.abz_rule_ltm_node_weights_fold(h, pout), L.ERR_ARG, "not made by abz_rule_ltm_unfold")
    # rules that are not a whole periodic grid, or hold no eigenvalues
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, npt, cub.syms, L.WANT_EIG)
    idx, w = abz.symptr_rule(npt, 3, cub.syms)
    irr, slab, halo = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, npt, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(irr)))
    L.check(lib.abz_ptr_rule_build_slab(dev.h, npt, 1, 3, L.WANT_EIG, C.byref(slab)))
    L.check(lib.abz_ptr_rule_build_slab(dev.h, npt, 1, 3, L.WANT_EIG, C.byref(halo)))
    L.check(lib.abz_rule_ltm_halo(halo))
    honly = abz.DeviceRule(dev, npt, None, L.WANT_H)
    for other, code in ((honly._h, L.ERR_ARG), (sym._h, L.ERR_UNSUPPORTED), (irr, L.ERR_UNSUPPORTED), (slab, L.ERR_UNSUPPORTED),
                        (halo, L.ERR_UNSUPPORTED)):
        refused(lib.abz_rule_ltm_node_weights(other, pE, 3, L.LTM_STATES, pout), code)
        refused(lib.abz_rule_ltm_node_weights_dot(other, pout), code)
        refused(lib.abz_rule_ltm_node_weights_fold(other, pout), code)
        base, nb, ne = C.c_void_p(1), C.c_int64(-1), C.c_int(-1)
        assert lib.abz_rule_ltm_node_weights_ptr(other, C.byref(base), C.byref(nb), C.byref(ne)) == 0
        assert (base.value, nb.value, ne.value) == (None, 0, 0)
    assert b"not a whole periodic grid" in lib.abz_last_error()
    # no resident weights: a fresh full grid with elements, and an unfolded rule
    other = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    other.ltm_elements(np.ones((1, npt ** 3, 1)))
    refused(lib.abz_rule_ltm_node_weights_dot(other._h, pout), L.ERR_ARG, "holds no integration weights")
    unf = sym.unfold()
    refused(lib.abz_rule_ltm_node_weights_fold(unf._h, pout), L.ERR_ARG, "holds no integration weights")
    with pytest.raises(ValueError, match="holds no weights"):
        unf.ltm_node_weights_fold()
    # valid calls afterwards still work
    assert lib.abz_rule_ltm_node_weights(h, pE, 3, L.LTM_STATES, pout) == 0
    assert np.array_equal(out[:3 * npt ** 3].reshape(3, npt ** 3, 1), kept) and np.all(out[3 * npt ** 3:] == -99.0)
    assert lib.abz_rule_destroy(irr) == 0 and lib.abz_rule_destroy(slab) == 0 and lib.abz_rule_destroy(halo) == 0
    # the Python mirror refuses a k-sharded rule
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        r = dev.rule(npt, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_node_weights(Es)
    finally:
        dev.kshard, dev.allreduce = None, None


# ---------------------------------------------------------------- 8. the front end
def test_integration_weights(abz):
    s = series_of(abz, "svo")
    a = 3.85856
    bz = abz.load_bz(abz.FBZ(), a * np.eye(3))
    cache = abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=8))
    rule = cache.cacheval
    eig = rule.export(x=False, w=False, eig=True)["eig"]
    nstates, tol = 1.0, 1e-10
    E_F, N_F = abz.dos.fermi_level(cache, nstates)
    W, E = abz.dos.integration_weights(cache, nstates=nstates)
    assert W.shape == (rule.nk, 3) and E == E_F
    # fermi_level: N crosses nstates inside (E_F - tol, E_F], so N(E_F) - nstates <= g tol (+ its own 1e-12 slack); sum W = N(E_F)
    g = rule.ltm(np.array([E_F]))[0]
    dev = abs(W.sum() - nstates)
    print(f"integration_weights: sum W - nstates = {W.sum() - nstates:.3e} (g tol = {g * tol:.1e}), sum W - N_F = {W.sum() - N_F:.3e}")
    assert dev <= g * tol + 1e-9 * max(1.0, nstates) and abs(W.sum() - N_F) <= 1e-9
    Wc, Ec = abz.dos.integration_weights(cache, nstates=nstates, correction=True)
    Eb, E_F2 = abz.dos.band_energy(cache, nstates)
    assert Ec == E_F2 == E_F
    check(np.array([np.einsum("kb,kb->", Wc, eig)]), np.array([Eb]), "einsum(W, eig) with the correction against band_energy")
    # a list of energies, the DOS weights, and a problem instead of a cache
    Es = np.array([12.3, 12.9])
    Wg, Eg = abz.dos.integration_weights(abz.DOSProblem(s, 0.0, bz), E=Es, kind="dos")
    assert Wg.shape == (2, 50 ** 3, 3) and np.array_equal(Eg, Es)
    check(Wg.sum(axis=(1, 2)), abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM()).u, "DOS weights of LTM() sum to its DOS")
    W1, E1 = abz.dos.integration_weights(cache, E=12.5)
    assert W1.shape == (rule.nk, 3) and E1 == 12.5
    with pytest.raises(ValueError, match="fold"):
        abz.dos.integration_weights(cache, E=12.5, fold=True)
    # LTM(symmetric=True): the weights on the irreducible nodes that were solved
    cub = abz.load_bz(abz.CubicSymIBZ(), a * np.eye(3))
    csym = abz.dos.init(abz.DOSProblem(s, 0.0, cub), abz.LTM(npt=8, symmetric=True))
    assert isinstance(csym.cacheval, abz.UnfoldedRule)
    Wf, Ef = abz.dos.integration_weights(csym, nstates=nstates, correction=True, fold=True)
    src = csym.cacheval.source
    assert Wf.shape == (src.nk, 3) and abs(Ef - E_F) <= 1e-9
    check(np.array([np.einsum("jb,jb->", Wf, src.export(x=False, w=False, eig=True)["eig"])]), np.array([abz.dos.band_energy(csym, nstates)[0]]),
          "folded weights against band_energy of the symmetric cache")


# ---------------------------------------------------------------- profiling
def test_node_weight_launches_are_profiled(abz):
    """One ProfScope of ABZ_K_LTM per call: around the groups of a weight call, around the two stages of a dot, around a fold."""
    L = abz._lib
    s = product_series(abz, orc.tb_integer(2))
    dev = s.device()
    src = abz.DeviceRule(dev, 8, model_sym_sets(abz, "int2", 2)["cubic"], L.WANT_EIG)
    unf = src.unfold()
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        dev.ctx.prof_reset()
        unf.ltm_node_weights(np.linspace(-3, 3, 16), export=False)
        ms, launches = dev.ctx.prof_read(L.K_LTM)
        assert launches == 1 and ms > 0.0
        unf.ltm_elements(np.ones((2, unf.nk, 1)))
        before = dev.ctx.prof_read(L.K_LTM)[1]
        unf.ltm_node_weights_dot()
        assert dev.ctx.prof_read(L.K_LTM)[1] == before + 1
        unf.ltm_node_weights_fold()
        assert dev.ctx.prof_read(L.K_LTM)[1] == before + 2
    finally:
        dev.ctx.prof_enable(False)
        unf.ltm_elements(None)

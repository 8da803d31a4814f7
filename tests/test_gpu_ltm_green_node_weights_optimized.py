"""Complex integration weights W_b(k; z) of the optimized tetrahedron method on the device
(abz_rule_ltm_green_node_weights_optimized; ltm_green_opt_cornerw_kernel of kernels_ltm_green_opt_nodew.hip and
ltm_opt_nodew_gather_kernel of ltm_opt_nodew_device.h) against the scatter-form restatement of tests/goptnodew_numpy.py, against
the shipped scans of abz_rule_ltm_green_optimized, and their bits, slabs, consumers (dot, fold, matrix), lifetime and refusals.

Parity bound: the restatement is fed the rule's own exported eigenvalues, so only summation order, FMA contraction and the form
of the 20-point product remain; test_ltm_green_node_weights_optimized_cpu.py shows that the f64 and the longdouble product agree
to 0.01 of the bound at every case and value of z used here.  The bound is the project's LTM parity bound on the O(1) quantity
nk W,   |nk W - nk ref| <= 1e-9 max(1, max|nk ref|)   on the real and on the imaginary part (close_nk of
test_gpu_ltm_green_node_weights.py).  A line stride beyond 2^31 doubles (ABZ_ERR_UNSUPPORTED) needs a grid no test can hold and
is not exercised."""
import ctypes as C
import gc

import numpy as np
import pytest

import abz_oracle as orc
import goptnodew_numpy as gonw
import ltm_numpy as ln
import unfold_numpy as un
from test_gpu_ltm import product_series
from test_gpu_ltm_green_matrix import bits
from test_gpu_ltm_green_node_weights import check, check_nk, on_nodes, read_gblock
from test_gpu_ltm_node_weights import read_block
from test_gpu_ltm_node_weights_optimized import books
from test_ltm_green_node_weights_optimized_cpu import PARITY_CASES, calls_for, model_coefficients, model_series, z_pool
from test_ltm_unfold_cpu import model_sym_sets

pytestmark = pytest.mark.gpu

SWITCH = "ABZ_LTM_OPTW_CHUNK_MB"


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


_SHARED = {}


def shared(abz, model, npt):
    """Per case, made once and left unchanged: the rule, its eigenvalues, the pool of z and the restatement's weights at the values
    the calls use"""
    key = (model, npt)
    if key not in _SHARED:
        rule = model_series(abz, model).device().rule(npt, None, abz._lib.WANT_EIG)
        eig = ln.rule_eigenvalues(rule)
        zs = z_pool(eig)
        calls = calls_for(model, npt)
        used = sorted({i for pick in calls.values() for i in pick})
        ref = np.zeros((len(zs), rule.nk, eig.shape[-1]), dtype=np.complex128)
        ref[used] = on_nodes(rule, gonw.node_weights(eig, zs[used]))
        ref.setflags(write=False)
        _SHARED[key] = dict(rule=rule, eig=eig, zs=zs, ref=ref, n=eig.shape[-1], calls=calls)
    return _SHARED[key]


# ---------------------------------------------------------------- 1. parity with the restatement
@pytest.mark.parametrize("model,npt", PARITY_CASES, ids=[f"{m}-{p}" for m, p in PARITY_CASES])
def test_optimized_green_node_weights_match_restatement(abz, model, npt):
    sh = shared(abz, model, npt)
    rule, zs, ref, n = sh["rule"], sh["zs"], sh["ref"], sh["n"]
    worst = 0.0
    for label, pick in sh["calls"].items():
        W = rule.ltm_green_node_weights_optimized(zs[pick])
        assert W.shape == (len(pick), rule.nk, n)
        worst = max(worst, check_nk(W, ref[pick], rule.nk, f"optimized {model} npt={npt} {label}"))
        assert rule.ltm_green_node_weights_ptr()[2] == len(pick)
    print(f"optimized green nodew parity {model} npt={npt}: worst deviation / bound = {worst:.3e}")


@pytest.mark.parametrize("model,npt", [(3, 5), (33, 3)])
def test_padding_columns_are_plus_zero_and_the_block_is_the_export(abz, model, npt):
    sh = shared(abz, model, npt)
    rule, zs, n = sh["rule"], sh["zs"], sh["n"]
    pick = sh["calls"]["three"]
    W = rule.ltm_green_node_weights_optimized(zs[pick])
    block = read_gblock(abz, rule).copy()
    assert np.all(block[:, :, npt:] == 0.0) and not np.any(np.signbit(block[:, :, npt:]))
    got = block[:, :, :npt].reshape(npt ** 2, len(pick), 2, n, npt).transpose(1, 0, 4, 3, 2).reshape(len(pick), rule.nk, n, 2)
    assert np.array_equal(np.ascontiguousarray(got).view(np.complex128)[..., 0], W)


# ---------------------------------------------------------------- 2. sums against the shipped scans
@pytest.mark.parametrize("model,npt", [(3, 5), ("svo", 6)])
def test_optimized_green_node_weights_against_the_shipped_scans(abz, model, npt):
    sh = shared(abz, model, npt)
    rule, zs, eig, n = sh["rule"], sh["zs"], sh["eig"], sh["n"]
    A = np.random.default_rng(2).standard_normal((16, rule.nk, n))
    rule.ltm_elements(A)
    e = eig.reshape(rule.nk, n)
    for label, pick in sh["calls"].items():
        z = zs[pick]
        tr = rule.ltm_green_optimized(z)
        scan = rule.ltm_green_optimized(z, elements="attached")  # [nz, 16]
        energy = rule.ltm_green_optimized(z, elements="energy")[:, 0]
        W = rule.ltm_green_node_weights_optimized(z)
        check(W.sum(axis=(1, 2)), tr, f"optimized {model} {label} sum of the weights against tr G")
        check(np.einsum("zkb,ckb->zc", W, A), scan, f"optimized {model} {label} einsum(W, A) against the scan")
        dot = rule.ltm_green_node_weights_dot()
        assert dot.shape == (len(pick), 16) and dot.dtype == np.complex128
        check(dot, scan, f"optimized {model} {label} dot against the scan")
        check(np.einsum("zkb,kb->z", W, e), energy, f"optimized {model} {label} einsum(W, e) against elements='energy'")
    rule.ltm_elements(None)


# ---------------------------------------------------------------- 3. bits
@pytest.mark.parametrize("model,npt", [(3, 5), ("svo", 6)])
def test_optimized_green_node_weights_repeat_conjugate_and_groups(abz, model, npt):
    sh = shared(abz, model, npt)
    rule, zs = sh["rule"], sh["zs"]
    for pick in sh["calls"].values():
        a = rule.ltm_green_node_weights_optimized(zs[pick])
        block_a = read_gblock(abz, rule).copy()
        b = rule.ltm_green_node_weights_optimized(zs[pick])
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(block_a, read_gblock(abz, rule))  # two calls, the same bits
        c = rule.ltm_green_node_weights_optimized(np.conj(zs[pick]))
        assert np.array_equal(bits(c), bits(np.conj(a)))  # W(conj z) = conj W(z), to the bit
    assert rule.ltm_green_node_weights_optimized(zs[:5], export=False) is None and rule.ltm_green_node_weights_ptr()[2] == 5
    # a value inside a call of 8 against the same value alone
    pick = sh["calls"]["eight"]
    W8 = rule.ltm_green_node_weights_optimized(zs[pick])
    scale = max(1.0, float(np.abs(rule.nk * W8).max()))
    worst = 0.0
    for j, i in enumerate(pick):
        W1 = rule.ltm_green_node_weights_optimized(zs[i:i + 1])[0]
        worst = max(worst, float(np.abs(rule.nk * (W8[j] - W1)).max()))
    print(f"{model} npt={npt}: a value inside a call of 8 against alone: nk |dW| = {worst:.2e} (bound {1e-13 * scale:.1e}; zero: {worst == 0.0})")
    assert worst <= 1e-13 * scale


def test_optimized_green_node_weights_do_not_depend_on_the_chunk(abz, monkeypatch):
    """npt = 17, 3 bands: a plane of cells takes 24 x 3 x 8 x 289 B = 166 KB per real set, a value of z two sets.  Cap 1 MB: slabs of
    one plane (many); 4 MB: slabs of 9 planes (a few); no cap: one slab of wrapped planes.  GPU bits against GPU bits; the block under
    the cap of 1 MB is also set against the restatement."""
    model, npt = 3, 17
    rule = model_series(abz, model).device().rule(npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    zs = z_pool(eig)
    calls = [[12], [21, 16, 7]]
    got = {}
    try:
        for cap in ("1", "4", None):
            if cap is None:
                monkeypatch.delenv(SWITCH, raising=False)
            else:
                monkeypatch.setenv(SWITCH, cap)
            got[cap] = [rule.ltm_green_node_weights_optimized(zs[pick]) for pick in calls]
    finally:
        monkeypatch.delenv(SWITCH, raising=False)
    for cap in ("1", "4"):
        for a, b in zip(got[cap], got[None]):
            assert np.array_equal(bits(a), bits(b)), cap
    two = [16, 7]
    check_nk(got["1"][1][1:], on_nodes(rule, gonw.node_weights(eig, zs[two])), rule.nk, "npt=17 under a cap of 1 MB against the restatement")


# ---------------------------------------------------------------- 4. unfolded rules and the fold
def test_optimized_green_node_weights_of_an_unfolded_rule_and_their_fold(abz):
    L = abz._lib
    model, npt = "svo", 6
    s = model_series(abz, model)
    dev = s.device()
    syms = model_sym_sets(abz, "svo", 3)["cubic"]
    src = abz.DeviceRule(dev, npt, syms, L.WANT_EIG)
    unf = src.unfold()
    full = dev.rule(npt, None, L.WANT_EIG)
    eig = ln.rule_eigenvalues(unf)
    n, nk, nirr = eig.shape[-1], unf.nk, src.nk
    zs = z_pool(eig)[calls_for(model, npt)["eight"]]
    node_of = un.orbit_map(npt, 3, syms, src.export(eig=True)["x"])  # the orbits on the host, from the exported nodes and the matrices
    W = unf.ltm_green_node_weights_optimized(zs)
    check_nk(W, full.ltm_green_node_weights_optimized(zs), nk, "svo npt=6 unfolded against the full build")
    check_nk(W, on_nodes(unf, gonw.node_weights(eig, zs)), nk, "svo npt=6 unfolded against the restatement")
    fold = unf.ltm_green_node_weights_fold()
    assert fold.shape == (len(zs), nirr, n) and fold.dtype == np.complex128
    host = np.zeros_like(fold)
    np.add.at(host, (slice(None), node_of), W)
    # an orbit holds at most 48 points: the bound on nk W, for sums of up to 48 of them
    check_nk(fold, host, nk, "svo npt=6 fold against host orbit sums of the export")
    assert np.array_equal(bits(fold), bits(unf.ltm_green_node_weights_fold()))


# ---------------------------------------------------------------- 5. the matrix G_pq(z)
@pytest.mark.parametrize("n,npt", [(3, 5), (9, 5), (17, 3)])
def test_green_matrix_from_the_optimized_weights(abz, n, npt):
    L = abz._lib
    rule = abz.DeviceRule(model_series(abz, n).device(), npt, None, L.WANT_H | L.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    zs = z_pool(eig)[[7, 16, 12, 0, 19]]
    G = rule.ltm_green_node_weights_matrix(zs, optimized=True)
    assert G.shape == (len(zs), n, n) and G.dtype == np.complex128 and np.all(np.isfinite(bits(G)))
    check(np.trace(G, axis1=1, axis2=2), rule.ltm_green_optimized(zs), f"optimized matrix n={n} trace against ltm_green_optimized")
    orb = list(range(min(n, 16)))
    rule.ltm_orbitals(orb)
    check(np.einsum("zpp->zp", G)[:, :len(orb)], rule.ltm_green_optimized(zs, elements="attached"),
          f"optimized matrix n={n} diagonal against ltm_green_optimized of the orbital weights")
    rule.ltm_elements(None)
    Gc = rule.ltm_green_node_weights_matrix(np.conj(zs), optimized=True)
    assert np.array_equal(bits(np.conj(G.transpose(0, 2, 1))), bits(Gc))  # G(z)^dagger = G(conj z), to the bit
    assert np.array_equal(bits(G), bits(rule.ltm_green_node_weights_matrix(zs, optimized=True)))
    assert np.array_equal(bits(rule.ltm_green_node_weights_matrix()), bits(G))  # the resident (optimized) weights without zs
    with pytest.raises(ValueError, match="optimized=True"):
        rule.ltm_green_node_weights_matrix(optimized=True)
    rule.close()


def test_green_local_fused_optimized_front_end(abz):
    s = model_series(abz, 3)
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    cache = abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=6, optimized=True))
    zs = np.array([0.3 + 1e-2j, -0.8 + 0.2j, 1.1 - 1e-3j])
    F = abz.dos.green_local_fused(cache, zs, optimized=True)
    assert F.shape == (3, 3, 3)
    check(np.trace(F, axis1=1, axis2=2), abz.dos.green_trace(cache, zs, optimized=True), "green_local_fused(optimized=True) traces to green_trace")
    # the default is the linear rule whatever the cache's algorithm is: another rule, and today's bits
    Fl = abz.dos.green_local_fused(cache, zs)
    assert np.array_equal(bits(Fl), bits(abz.dos.green_local_fused(cache, zs, optimized=False)))
    assert np.array_equal(bits(Fl), bits(cache.cacheval.ltm_green_node_weights_matrix(zs)))
    diff = float(np.abs(F - Fl).max())
    print(f"npt = 6: max |G_opt - G_lin| = {diff:.3e}")
    assert diff > 1e-4
    W, zl = abz.dos.green_weights(cache, zs, optimized=True)
    assert W.shape == (3, 216, 3) and np.array_equal(zl, zs)
    check(W.sum(axis=(1, 2)), abz.dos.green_trace(cache, zs, optimized=True), "green_weights(optimized=True) sum to green_trace")
    W1, z1 = abz.dos.green_weights(cache, zs[1], optimized=True)
    assert np.array_equal(bits(W1), bits(W[1])) and z1 == zs[1]
    Wl, _ = abz.dos.green_weights(cache, zs)
    assert np.array_equal(bits(Wl), bits(cache.cacheval.ltm_green_node_weights(zs)))
    # a k-sharded series is refused before anything is built
    dev = s.device()
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        for f in (abz.dos.green_weights, abz.dos.green_local_fused):
            with pytest.raises(NotImplementedError, match="k-sharded"):
                f(abz.DOSProblem(s, 0.0, bz), zs, optimized=True)
        r = dev.rule(6, None, abz._lib.WANT_EIG)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_green_node_weights_optimized(zs)
    finally:
        dev.kshard, dev.allreduce = None, None


# ---------------------------------------------------------------- 6. lifetime
def test_optimized_complex_weights_and_the_other_blocks(abz):
    """The real weights are untouched (pointer, size, contents); the call replaces a linear complex block and is replaced by one; a
    rebuild drops the block."""
    sh = shared(abz, 3, 5)
    zs, n = sh["zs"], sh["n"]
    rule = model_series(abz, 3).device().rule(5, None, abz._lib.WANT_EIG)  # (a rule of its own: it is rebuilt below)
    pick = sh["calls"]["three"]
    Es = np.array([0.1, 0.4, -0.2])
    rule.ltm_node_weights(Es, export=False)
    pr, br = rule.ltm_node_weights_ptr(), read_block(abz, rule).copy()
    lin = rule.ltm_green_node_weights(zs[pick])
    assert rule.ltm_green_node_weights_ptr()[2] == 3
    opt = rule.ltm_green_node_weights_optimized(zs[pick[:2]])
    assert rule.ltm_green_node_weights_ptr()[1:] == (8 * 25 * 2 * 2 * n * 16, 2)  # lines x values x (re, im) x bands x padded row
    assert float(np.abs(rule.nk * (opt - lin[:2])).max()) > 1e-3  # the block is the optimized one now
    assert rule.ltm_node_weights_ptr() == pr and np.array_equal(read_block(abz, rule), br)
    again = rule.ltm_green_node_weights(zs[pick])
    assert np.array_equal(bits(again), bits(lin)) and rule.ltm_green_node_weights_ptr()[2] == 3
    assert np.array_equal(bits(rule.ltm_green_node_weights_optimized(zs[pick[:2]])), bits(opt))
    assert rule.ltm_node_weights_ptr() == pr and np.array_equal(read_block(abz, rule), br)
    rule.rebuild()
    assert rule.ltm_green_node_weights_ptr() == (0, 0, 0)
    with pytest.raises(ValueError, match="holds no weights"):
        rule.ltm_green_node_weights_matrix()


def test_optimized_green_node_weights_are_accounted(abz):
    """abz_mem_info counts the block, 8 npt^2 2 nz n row bytes, as the rule's; a replacement does not add one; a rebuild drops it and
    keeps the context's scratch; destroying everything gives everything back."""
    L = abz._lib
    lib = L.lib()
    npt, n, nz = 6, 2, 3
    c = np.ascontiguousarray(model_coefficients(n)[0])
    dims, first, per = np.array([3, 3, 3], dtype=np.int32), np.array([-1, -1, -1], dtype=np.int32), np.ones(3)
    zs = np.array([0.1 + 0.1j, -0.3 - 0.2j, 0.2 + 1e-3j])
    pz = zs.view(np.float64).ctypes.data_as(L.c_f64p)
    block = 8 * npt ** 2 * 2 * nz * n * 16
    gc.collect()
    gc.disable()
    try:
        for attempt in range(2):  # the first round warms the allocator's pool: blocks, not bytes, could differ
            b0 = books(L, None)
            ctx, s, full = C.c_void_p(), C.c_void_p(), C.c_void_p()
            L.check(lib.abz_ctx_create(0, C.byref(ctx)))
            L.check(lib.abz_series_create(ctx, c.view(np.float64).ctypes.data_as(L.c_f64p), 3, dims.ctypes.data_as(L.c_i32p),
                                          first.ctypes.data_as(L.c_i32p), per.ctypes.data_as(L.c_f64p), n, C.byref(s)))
            L.check(lib.abz_ptr_rule_build(s, npt, 0, None, None, L.WANT_EIG, C.byref(full)))
            b1 = books(L, ctx)
            L.check(lib.abz_rule_ltm_green_node_weights_optimized(full, pz, nz, None))  # (the scratch exists from here on)
            bA = books(L, ctx)
            assert bA[2] >= 8 * 24 * n * 2 * npt ** 3  # one value of z, the whole grid in one slab
            base, nb, cnt = C.c_void_p(), C.c_int64(-1), C.c_int(-1)
            L.check(lib.abz_rule_ltm_green_node_weights_ptr(full, C.byref(base), C.byref(nb), C.byref(cnt)))
            assert (nb.value, cnt.value) == (block, nz)
            L.check(lib.abz_rule_ltm_green_node_weights_optimized(full, pz, nz, None))  # replaced, not added
            assert books(L, ctx)[1:] == bA[1:]
            L.check(lib.abz_rule_rebuild(full))  # drops the block, not the scratch
            bB = books(L, ctx)
            assert bB[1] == bA[1] - 1 and bB[2] >= bA[2]
            L.check(lib.abz_rule_ltm_green_node_weights_optimized(full, pz, nz, None))
            bC = books(L, ctx)
            assert bC[1] == bB[1] + 1 and block <= bC[0] - bB[0] <= 2 * block and bC[2] == bB[2]
            assert lib.abz_rule_destroy(full) == 0  # with the weights resident
            assert lib.abz_series_destroy(s) == 0
            assert lib.abz_ctx_destroy(ctx) == 0
            b5 = books(L, None)
            print(f"books (live bytes, live blocks, scratch): start {b0}, rule {b1}, weights {bA}, rebuilt {bB}, weights again {bC}, end {b5}")
            if attempt == 1:
                assert b5[:2] == b0[:2]
    finally:
        gc.enable()


# ---------------------------------------------------------------- 7. refusals
def test_optimized_green_node_weight_refusals(abz):
    """One row per error code of the header: the code and its text, `out` untouched, both weight blocks and the attached elements
    as they were, and a valid call afterwards."""
    L = abz._lib
    lib = L.lib()
    sh = shared(abz, 3, 4)
    npt, n = 4, 3
    nk = npt ** 3
    s = model_series(abz, 3)
    dev = s.device()
    full = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    h = full._h
    zs = np.array([0.5 + 0.1j, 1.5 - 1e-3j, -0.5 + 1e-4j])
    Es = np.array([0.5, 1.5])
    pz = zs.view(np.float64).ctypes.data_as(L.c_f64p)
    out = np.full(2 * 9 * nk * n, -99.0)
    pout = out.ctypes.data_as(L.c_f64p)
    A = np.random.default_rng(2).standard_normal((2, nk, n))
    full.ltm_elements(A)
    kept = full.ltm_green_node_weights(zs)  # a resident complex block (the linear rule's)
    full.ltm_node_weights(Es, export=False)
    f = lib.abz_rule_ltm_green_node_weights_optimized

    def state():
        pc, pr = full.ltm_green_node_weights_ptr(), full.ltm_node_weights_ptr()
        return (pc, read_gblock(abz, full).copy(), pr, read_block(abz, full).copy(), full.ltm_elements_export())

    st = state()

    def refused(rc, code, words=None):
        msg = lib.abz_last_error().decode()
        assert rc == code and len(msg) > 0, (rc, code, msg)
        assert words is None or words in msg, msg
        assert np.all(out == -99.0)  # nothing was written
        # both weight blocks (pointer, size, contents) and the attached elements are what they were
        now = state()
        assert now[0] == st[0] and now[2] == st[2] and all(np.array_equal(now[i], st[i]) for i in (1, 3, 4)), msg

    f64 = lambda a: np.ascontiguousarray(a).view(np.float64).ctypes.data_as(L.c_f64p)
    # ABZ_ERR_ARG
    assert f(None, pz, 3, pout) == L.ERR_ARG and b"null rule handle" in lib.abz_last_error() and np.all(out == -99.0)
    refused(f(h, None, 3, pout), L.ERR_ARG, "null z")
    for nz in (0, 9, -1):
        refused(f(h, pz, nz, pout), L.ERR_ARG, "outside 1..8")
    refused(f(h, f64(np.array([0.5 + 0.1j, 0.7 + 0j])), 2, pout), L.ERR_ARG, "is real")
    for bad in (np.nan + 0.1j, 0.1 + 1j * np.inf, complex(np.inf, 0.1)):
        refused(f(h, f64(np.array([0.5 + 0.1j, bad])), 2, pout), L.ERR_ARG, "not finite")
    honly = abz.DeviceRule(dev, npt, None, L.WANT_H)
    refused(f(honly._h, pz, 3, pout), L.ERR_ARG, "ABZ_WANT_EIG")
    honly.close()
    # ABZ_ERR_UNSUPPORTED: d = 2; a slab without and with its halo plane; irreducible nodes
    s2 = product_series(abz, orc.tb_integer(2))
    flat = abz.DeviceRule(s2.device(), 8, None, L.WANT_EIG)
    refused(f(flat._h, pz, 3, pout), L.ERR_UNSUPPORTED, "d = 2")
    with pytest.raises(NotImplementedError, match="d = 3"):
        flat.ltm_green_node_weights_optimized(zs)
    with pytest.raises(NotImplementedError, match="d = 3"):
        flat.ltm_green_node_weights_matrix(zs, optimized=True)
    flat.close()
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    idx, w = abz.symptr_rule(npt, 3, cub.syms)
    irr, slab, halo = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, npt, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(irr)))
    L.check(lib.abz_ptr_rule_build_slab(dev.h, npt, 1, 3, L.WANT_EIG, C.byref(slab)))
    L.check(lib.abz_ptr_rule_build_slab(dev.h, npt, 1, 3, L.WANT_EIG, C.byref(halo)))
    L.check(lib.abz_rule_ltm_halo(halo))
    for other in (irr, slab, halo):
        refused(f(other, pz, 3, pout), L.ERR_UNSUPPORTED, "not a whole periodic grid")
        base, nb, cnt = C.c_void_p(1), C.c_int64(-1), C.c_int(-1)
        assert lib.abz_rule_ltm_green_node_weights_ptr(other, C.byref(base), C.byref(nb), C.byref(cnt)) == 0
        assert (base.value, nb.value, cnt.value) == (None, 0, 0)
    assert lib.abz_rule_destroy(irr) == 0 and lib.abz_rule_destroy(slab) == 0 and lib.abz_rule_destroy(halo) == 0
    # the Python mirror's own argument checks
    with pytest.raises(ValueError, match="takes 1..8"):
        full.ltm_green_node_weights_optimized(np.arange(9) + 0.1j)
    with pytest.raises(ValueError, match="real value"):
        full.ltm_green_node_weights_optimized([0.3])
    # a valid call afterwards works, and writes what it should and no more
    assert f(h, pz, 3, pout) == 0
    m = 2 * 3 * nk * n
    got = out[:m].view(np.complex128).reshape(3, nk, n)
    assert np.all(out[m:] == -99.0)
    check_nk(got, on_nodes(full, gonw.node_weights(sh["eig"], zs)), nk, "a valid call after the refusals")
    assert float(np.abs(nk * (got - kept)).max()) > 1e-3  # the complex block is the optimized one now
    end = state()
    assert end[0][1:] == st[0][1:] and end[2] == st[2] and np.array_equal(end[3], st[3]) and np.array_equal(end[4], st[4])
    full.close()


# ---------------------------------------------------------------- 8. profiling
def test_optimized_green_node_weight_launches_are_profiled(abz):
    """One ProfScope of ABZ_K_LTM around the launches of a call, whatever the number of groups and slabs."""
    L = abz._lib
    s = model_series(abz, 3)
    dev = s.device()
    rule = dev.rule(8, None, L.WANT_EIG)
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        dev.ctx.prof_reset()
        rule.ltm_green_node_weights_optimized(np.linspace(-3, 3, 7) + 0.1j, export=False)
        ms, launches = dev.ctx.prof_read(L.K_LTM)
        assert launches == 1 and ms > 0.0
    finally:
        dev.ctx.prof_enable(False)

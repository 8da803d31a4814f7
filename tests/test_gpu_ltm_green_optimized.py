"""Green's functions of the optimized tetrahedron method on the device (abz_rule_ltm_green_optimized; ltm_green_opt_kernel,
kernels_ltm_green_opt.hip) against the restatement of tests/goptltm_numpy.py, a composition of optltm_numpy.py (the projection
from its definition) and gltm_numpy.py / gwltm_numpy.py (the evaluation rule) that reads no table of the kernels.

Parity bound: the restatement is fed the rule's own exported eigenvalues and the very elements that are attached, so only
summation order, FMA contraction and the form of the product (the kernel adds sum_j P_mj (x_j - x_m) to x_m) remain; the cases
and z lists are those of test_ltm_green_optimized_cpu.py, whose f64 and longdouble evaluations agree to 1e-10 of the scale.  The
bound is the project's LTM parity bound, |u - ref| <= 1e-9 max(1, max|ref|) (`close` of test_gpu_ltm.py)."""
import ctypes as C

import numpy as np
import pytest

import abz_oracle as orc
import goptltm_numpy as gon
import ltm_numpy as ln
import optltm_numpy as on
from test_gpu_ltm import close, product_series
from test_ltm_optimized_cpu import GRIDS, SEEDS, case_coefficients, case_elements

pytestmark = pytest.mark.gpu

# values of z per launch of a group of 1, 2 and 4 components (green_w_chunk of ltm_green_device.h; the trace is a group of 1)
CHUNK = {1: 512, 2: 291, 4: 154}


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def check(u, ref, what):
    u, ref = np.asarray(u), np.asarray(ref)
    assert u.shape == ref.shape and np.all(np.isfinite(np.ascontiguousarray(u).view(np.float64))), (what, u.shape, ref.shape)
    dev, bound = close(u, ref)
    print(f"goptltm {what}: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)
    return dev / bound


def case_rule(abz, n, npt):
    c, first = case_coefficients(n)
    s = abz.FourierSeries(c, period=1.0, first=first, ndim=3)
    return s, s.device().rule(npt, None, abz._lib.WANT_EIG)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------- parity with the restatement
@pytest.mark.parametrize("n", sorted(SEEDS))
@pytest.mark.parametrize("npt", GRIDS)
def test_green_optimized_matches_restatement(abz, n, npt):
    s, rule = case_rule(abz, n, npt)
    eig = ln.rule_eigenvalues(rule)
    A = case_elements(n, npt)
    worst = 0.0
    for label, zs in gon.z_lists(eig).items():
        what = f"n={n} npt={npt} {label}"
        worst = max(worst, check(rule.ltm_green_optimized(zs), gon.green(eig, None, zs), f"{what} trace"))
        worst = max(worst, check(rule.ltm_green_optimized(zs, elements="energy"), gon.green(eig, "energy", zs), f"{what} energy"))
        # the components are independent: one restatement of all 5 serves the calls with 1, 3 and 5 of them (group tails 1 | 2 + 1 | 4 + 1)
        ref = gon.green(eig, A.reshape((5,) + eig.shape), zs)
        for ncomp in (1, 3, 5):
            worst = max(worst, check(rule.ltm_green_optimized(zs, elements=A[:ncomp]), ref[:, :ncomp], f"{what} elements {ncomp}"))
    rule.ltm_elements(None)
    print(f"goptltm parity n={n} npt={npt}: worst deviation / bound = {worst:.3e}")


# ---------------------------------------------------------------- identities on the device
@pytest.mark.parametrize("n", sorted(SEEDS))
def test_green_optimized_identities(abz, n):
    s, rule = case_rule(abz, n, 7)
    eig = ln.rule_eigenvalues(rule)
    zs = gon.z_lists(eig)["generic"]
    tr = rule.ltm_green_optimized(zs)
    # sum_i W_i = J and A' = 1 exactly: attached ones give the trace
    ones = rule.ltm_green_optimized(zs, elements=np.ones((1, rule.nk, n)))[:, 0]
    dev = np.abs(ones - tr).max()
    print(f"n={n} elements == 1 against the trace: {dev:.2e}")
    assert dev <= 1e-12 * max(1.0, np.abs(tr).max())
    rule.ltm_elements(None)
    # sum_i x_i W_i = z J - 1
    check(rule.ltm_green_optimized(zs, elements="energy")[:, 0], zs * tr - n, f"n={n} energy against z tr G - n")


def test_green_optimized_flat_band(abz):
    """the flat band of test_optimized_flat_band: e' = v to the bit, every simplex is 1 / (z - v)"""
    c = np.zeros((3, 3, 3, 1, 1), dtype=np.complex128)
    c[1, 1, 1, 0, 0] = 0.25
    s = abz.FourierSeries(c, period=1.0, first=(-1, -1, -1), ndim=3)
    rule = s.device().rule(6, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    v = float(eig.reshape(-1)[0])
    assert np.all(eig == v)
    zs = np.array([v + x + 1j * y for x in (0.0, 0.3, -2.0) for y in (0.5, 1e-2, 1e-5, 1e-8, -1e-8, -0.5)])
    G = rule.ltm_green_optimized(zs)
    rel = np.abs(G - 1.0 / (zs - v)) * np.abs(zs - v)
    print(f"flat band: worst relative deviation from 1 / (z - v) {rel.max():.2e}")
    assert rel.max() <= 1e-14


def test_green_optimized_conjugate_repeatable_and_any_order(abz):
    s, rule = case_rule(abz, 3, 8)
    eig = ln.rule_eigenvalues(rule)
    zs = gon.z_lists(eig)["generic"]
    rule.ltm_elements(case_elements(3, 8)[:3])
    order = np.array([4, 0, 7, 7, 2, 19, 0, 11])  # permuted, with duplicates
    for el in (None, "energy", "attached"):
        a, b = rule.ltm_green_optimized(zs, elements=el), rule.ltm_green_optimized(zs, elements=el)
        assert np.array_equal(bits(a), bits(b)), el
        # Im z < 0 is the conjugate of conj z, bit for bit
        assert np.array_equal(bits(rule.ltm_green_optimized(np.conj(zs), elements=el)), bits(np.conj(a))), el
        # every z is summed in the same order whatever list it came in
        p = rule.ltm_green_optimized(zs[order], elements=el)
        assert np.array_equal(bits(p), bits(a[order])), el
        for i in (0, 7, 19):
            assert np.array_equal(bits(rule.ltm_green_optimized(zs[i:i + 1], elements=el)), bits(a[i:i + 1])), (el, i)
    rule.ltm_elements(None)


def test_green_optimized_lists_that_cross_a_chunk(abz):
    """A list one longer than the z chunk of every component group, at npt = 3: each z has the bits it has in a short list."""
    s, rule = case_rule(abz, 1, 3)
    eig = ln.rule_eigenvalues(rule)
    lo, hi = float(eig.min()), float(eig.max())
    A = case_elements(1, 3)
    # (elements, the groups they run in); 4 components run in the chunk of 4, 2 in that of 2, the rest in that of 1
    for el, ch in ((None, CHUNK[1]), ("energy", CHUNK[1]), (A[:1], CHUNK[1]), (A[:2], CHUNK[2]), (A[:4], CHUNK[4])):
        zs = np.linspace(lo - 0.1, hi + 0.1, ch + 1) + 3e-2j
        u = rule.ltm_green_optimized(zs, elements=el)
        assert np.all(np.isfinite(u.view(np.float64)))
        el2 = el if el is None or isinstance(el, str) else "attached"
        for sl in (slice(0, 5), slice(ch - 3, ch), slice(ch - 1, ch + 1), slice(ch, ch + 1)):
            assert np.array_equal(bits(rule.ltm_green_optimized(zs[sl], elements=el2)), bits(u[sl])), (el2, ch, sl)
    # and against the restatement, thinned
    zs = np.linspace(lo - 0.1, hi + 0.1, CHUNK[4] + 1) + 3e-2j
    check(rule.ltm_green_optimized(zs, elements=A[:4])[::11], gon.green(eig, A[:4].reshape((4,) + eig.shape), zs[::11]), "chunk list")
    rule.ltm_elements(None)


# ---------------------------------------------------------------- the limit eta -> 0
def test_green_optimized_tends_to_the_optimized_dos(abz):
    s, rule = case_rule(abz, 3, 8)
    eig = ln.rule_eigenvalues(rule)
    lo, hi = float(eig.min()), float(eig.max())
    Es = lo + (hi - lo) * np.array([0.3, 0.5, 0.7])
    ce = gon.corners(eig)[0]
    gap = np.abs(ce.reshape(-1)[None, :] - Es[:, None]).min()
    assert gap > 1e-4, gap  # away from any e' corner, where g has its kinks
    eta = 1e-6
    # what the restatement shows for the same comparison, times 10 for the order of summation
    ref_g = on.optltm(eig, None, Es, False)[:, 0]
    ref_b = -gon.green(eig, None, Es + 1j * eta).imag / np.pi
    tol = 10.0 * np.abs(ref_b - ref_g).max()
    g = rule.ltm_optimized(Es)
    b = -rule.ltm_green_optimized(Es + 1j * eta).imag / np.pi
    print(f"eta = {eta}: restatement |broadened - g| {np.abs(ref_b - ref_g).max():.3e}, device {np.abs(b - g).max():.3e}, tolerance {tol:.3e}; "
          f"nearest e' corner {gap:.2e}")
    assert np.abs(b - g).max() <= tol
    # the linear trace does not tend to it
    assert np.abs(-rule.ltm_green(Es + 1j * eta).imag / np.pi - g).max() > 100 * tol


# ---------------------------------------------------------------- unfolded rule and the Python front end
def test_green_optimized_on_an_unfolded_rule(abz):
    L = abz._lib
    s = product_series(abz, orc.tb_integer(3))
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    full = s.device().rule(8, None, L.WANT_EIG)
    zs = np.array([-5.5 + 0.5j, -1.3 + 1e-2j, 0.4 + 1e-4j, 2.2 - 1e-3j, 7.0 + 1e-2j])
    cache = abz.dos.init(abz.DOSProblem(s, 0.0, cub), abz.LTM(npt=8, symmetric=True))
    check(abz.dos.green_trace(cache, zs, optimized=True), full.ltm_green_optimized(zs), "LTM(symmetric) cache, optimized trace")
    check(full.ltm_green_optimized(zs), gon.green(ln.rule_eigenvalues(full), None, zs), "int3 against the restatement")


def test_green_optimized_front_end(abz):
    L = abz._lib
    c, first = case_coefficients(3)
    s = abz.FourierSeries(c, period=1.0, first=first, ndim=3)
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    rule = s.device().rule(8, None, L.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    zs = gon.z_lists(eig)["generic"][::3]
    f = lambda x, e: np.stack([e, np.cos(2 * np.pi * x[:, :1]) + 0 * e])
    ex = rule.export(x=True, w=False, eig=True)
    tr_opt, tr_lin = rule.ltm_green_optimized(zs), rule.ltm_green(zs)
    en_opt, en_lin = rule.ltm_green_optimized(zs, elements="energy"), rule.ltm_green(zs, elements="energy")
    Af = f(ex["x"], ex["eig"])
    f_opt, f_lin = rule.ltm_green_optimized(zs, elements=Af), rule.ltm_green(zs, elements=Af)
    rule.ltm_elements(None)
    assert np.abs(tr_opt - tr_lin).max() > 1e-4  # two rules
    for optimized in (False, True):  # the cache's algorithm does not choose the rule of the Green's functions: the keyword does
        prob = abz.DOSProblem(s, 0.0, bz)
        cache = abz.dos.init(prob, abz.LTM(npt=8, optimized=optimized))
        assert np.array_equal(bits(abz.dos.green_trace(cache, zs, optimized=True)), bits(tr_opt))
        assert np.array_equal(bits(abz.dos.green_trace(cache, zs, optimized=False)), bits(tr_lin))
        assert np.array_equal(bits(abz.dos.green_trace(cache, zs)), bits(tr_lin))
        cache = abz.dos.init(prob, abz.LTM(npt=8, optimized=optimized, elements="energy"))
        assert np.array_equal(bits(abz.dos.green_weighted(cache, zs, optimized=True)), bits(en_opt))
        assert np.array_equal(bits(abz.dos.green_weighted(cache, zs, optimized=False)), bits(en_lin))
        assert np.array_equal(bits(abz.dos.green_weighted(cache, zs)), bits(en_lin))
        cache = abz.dos.init(prob, abz.LTM(npt=8, optimized=optimized, elements=f))
        assert np.array_equal(bits(abz.dos.green_weighted(cache, zs, optimized=True)), bits(f_opt))
        assert np.array_equal(bits(abz.dos.green_weighted(cache, zs)), bits(f_lin))
    rule.ltm_elements(None)  # (the caches share the device's rule of this grid and left their elements on it)
    with pytest.raises(ValueError):
        rule.ltm_green_optimized(zs, elements="attached")
    with pytest.raises(ValueError):
        rule.ltm_green_optimized(zs, elements="bands")
    with pytest.raises(ValueError, match="real"):
        rule.ltm_green_optimized([0.5])


# ---------------------------------------------------------------- refusals
def test_green_optimized_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s, full = case_rule(abz, 3, 8)
    dev = s.device()
    zs = np.array([0.5 + 1e-2j, 1.5 - 1e-3j])
    Es = np.array([0.5, 1.5])
    out = np.full(2 * 16, -99.0)
    pz, pout = zs.view(np.float64).ctypes.data_as(L.c_f64p), out.ctypes.data_as(L.c_f64p)
    ALL = (L.LTM_A_ONE, L.LTM_A_ENERGY, L.LTM_A_ELEMENTS)

    def refused(h, code, sources=ALL, nz=2, z=pz, o=pout):
        for source in sources:
            assert lib.abz_rule_ltm_green_optimized(h, source, z, nz, o) == code, (source, code)
            assert len(lib.abz_last_error()) > 0
            assert np.all(out == -99.0)  # nothing was launched or written

    before = (full.ltm_green(zs), full.ltm_optimized(Es), full.ltm(Es))
    # d = 2
    s2 = product_series(abz, orc.tb_integer(2))
    flat = abz.DeviceRule(s2.device(), 8, None, L.WANT_EIG)
    before2 = (flat.ltm_green(zs), flat.ltm(Es))
    refused(flat._h, L.ERR_UNSUPPORTED)
    assert b"d = 2" in lib.abz_last_error()
    with pytest.raises(NotImplementedError, match="d = 3"):
        flat.ltm_green_optimized(zs)
    # a slab, without and with its halo plane
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, 8, 2, 6, L.WANT_EIG, C.byref(slab)))
    refused(slab, L.ERR_UNSUPPORTED)
    L.check(lib.abz_rule_ltm_halo(slab))
    refused(slab, L.ERR_UNSUPPORTED)
    # irreducible nodes
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    idx, w = abz.symptr_rule(8, 3, cub.syms)
    irr = C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, 8, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(irr)))
    refused(irr, L.ERR_UNSUPPORTED)
    assert b"not a whole periodic grid" in lib.abz_last_error()
    # a pair rule: the linear trace serves it, this entry point does not open e'_c - e'_v
    pr = full.ltm_pairs((0, 1), (1, 2))
    pair_before = pr.ltm_green(zs)
    refused(pr._h, L.ERR_UNSUPPORTED)
    assert b"pair rule" in lib.abz_last_error()
    assert np.array_equal(bits(pr.ltm_green(zs)), bits(pair_before))
    pr.close()
    # a rule without eigenvalues
    honly = abz.DeviceRule(dev, 8, None, L.WANT_H)
    refused(honly._h, L.ERR_ARG)
    # the full grid: arguments
    h = full._h
    refused(h, L.ERR_ARG, sources=(5, -1))
    refused(h, L.ERR_ARG, sources=(L.LTM_A_ELEMENTS,))  # nothing attached
    assert b"no matrix elements" in lib.abz_last_error()
    for bad in (0.5 + 0.0j, complex(float("nan"), 1e-2), complex(0.5, float("inf")), complex(float("inf"), 1e-2), complex(0.5, float("nan"))):
        zb = np.array([0.5 + 1e-2j, bad])
        refused(h, L.ERR_ARG, sources=(L.LTM_A_ONE, L.LTM_A_ENERGY), z=zb.view(np.float64).ctypes.data_as(L.c_f64p))
    refused(h, L.ERR_ARG, nz=0)
    refused(h, L.ERR_ARG, z=None)
    refused(h, L.ERR_ARG, o=None)
    # the rules are as they were: the other scans return the same bits, a valid call works and writes its own results only
    after = (full.ltm_green(zs), full.ltm_optimized(Es), full.ltm(Es))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after))
    assert np.array_equal(bits(flat.ltm_green(zs)), bits(before2[0])) and np.array_equal(flat.ltm(Es), before2[1])
    eig = ln.rule_eigenvalues(full)
    assert lib.abz_rule_ltm_green_optimized(h, L.LTM_A_ONE, pz, 2, pout) == 0
    check(out[:4].view(np.complex128), gon.green(eig, None, zs), "a valid call after the refusals")
    assert np.all(out[4:] == -99.0)
    A = case_elements(3, 8)[:3]
    full.ltm_elements(A)
    assert lib.abz_rule_ltm_green_optimized(h, L.LTM_A_ELEMENTS, pz, 2, pout) == 0
    check(out[:12].view(np.complex128).reshape(2, 3), gon.green(eig, A.reshape((3,) + eig.shape), zs), "attached elements through the C call")
    assert np.all(out[12:] == -99.0)
    full.ltm_elements(None)
    assert lib.abz_rule_destroy(irr) == 0 and lib.abz_rule_destroy(slab) == 0
    # the Python mirror refuses a k-sharded rule before it asks the library
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        r = dev.rule(8, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_green_optimized(zs)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_green_optimized(zs, elements="energy")
    finally:
        dev.kshard, dev.allreduce = None, None


# ---------------------------------------------------------------- profiling
def test_green_optimized_launches_are_profiled(abz):
    """The launches are counted under K_LTM: one scope per (component group, chunk of z); groups of 4, 2 and 1 components."""
    L = abz._lib
    s, rule = case_rule(abz, 3, 8)
    dev = s.device()
    zs = np.linspace(-3, 3, 10) + 1e-2j
    rule.ltm_elements(case_elements(3, 8)[:3])
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        dev.ctx.prof_reset()
        rule.ltm_green_optimized(zs)
        rule.ltm_green_optimized(zs, elements="energy")
        ms, launches = dev.ctx.prof_read(L.K_LTM)
        assert launches == 2 and ms > 0.0
        rule.ltm_green_optimized(zs, elements="attached")  # 3 components: a group of 2 and a group of 1
        assert dev.ctx.prof_read(L.K_LTM)[1] == 2 + 2
        rule.ltm_green_optimized(np.linspace(-3, 3, CHUNK[2] + 1) + 1e-2j, elements="attached")  # 2 chunks of the 2, 1 of the 1
        assert dev.ctx.prof_read(L.K_LTM)[1] == 4 + 3
        assert dev.ctx.prof_read(L.K_GGR)[1] == 0
    finally:
        dev.ctx.prof_enable(False)
        rule.ltm_elements(None)

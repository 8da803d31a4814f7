"""Tetrahedron method with matrix elements and the Fermi level on the device (abz_rule_ltm_elements,
abz_rule_ltm_weighted, abz_rule_ltm_fermi; ltm_window_kernel with the LtmElems payload, kernels_ltm.hip) against the geometric restatement
of tests/wltm_numpy.py and against the shipped unweighted scan.

Parity bound: the restatement is fed the rule's own exported eigenvalues and the very elements that are attached, so
only summation order and FMA contraction remain; the bound is the project's LTM / GGR parity bound,
|u - ref| <= 1e-9 max(1, max|ref|) (test_gpu_ltm.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import abz_oracle as orc
import ltm_numpy as ln
import wltm_numpy as wn
from test_gpu_ltm import GOLD, close, energy_lists, make_case, product_series
from test_ltm_cpu import MODELS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def on_grid(rule, A):
    """elements [ncomp, nk, n] -> [ncomp] + [npt]*d + [n], the shape ln.rule_eigenvalues gives the eigenvalues"""
    d = rule.dev.s.d
    return A.reshape((A.shape[0],) + (rule.npt,) * d + (A.shape[-1],))


def check(u, ref, what):
    assert u.shape == ref.shape and np.all(np.isfinite(u)), (what, u.shape, ref.shape)
    dev, bound = close(u, ref)
    print(f"wltm {what}: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)
    return dev / bound


def svo(abz):
    return abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))


# ---------------------------------------------------------------- parity with the restatement
@pytest.mark.parametrize("name", ["int1", "int2", "graphene", "int3", "svo", "syn6", "syn16", "syn33"])
def test_weighted_ltm_matches_restatement(abz, name):
    s, npt = make_case(abz, name)
    rule = s.device().rule(npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    n = eig.shape[-1]
    rng = np.random.default_rng(17)
    A = rng.standard_normal((16, rule.nk, n))
    lists = energy_lists(eig, np.random.default_rng(5))
    # the components are independent: one restatement of all 16 serves the calls with 1, 3 and 16 of them
    refs = {label: wn.wltm(eig, on_grid(rule, A), Es) for label, Es in lists.items()}
    worst = 0.0
    for ncomp in (1, 3, 16):
        rule.ltm_elements(A[:ncomp])
        for label, Es in lists.items():
            for states in (False, True):
                u = rule.ltm(Es, states=states, elements="attached")
                ref = refs[label][1 if states else 0][:, :ncomp]
                worst = max(worst, check(u, ref, f"{name} npt={npt} {label} ncomp={ncomp} {'N' if states else 'g'}"))
    rule.ltm_elements(None)
    print(f"wltm parity {name}: worst deviation / bound = {worst:.3e}")


# ---------------------------------------------------------------- against the shipped scan
@pytest.mark.parametrize("name", ["int2", "svo", "syn6"])
def test_weighted_ltm_against_the_shipped_scan(abz, name):
    s, npt = make_case(abz, name)
    rule = s.device().rule(npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    n = eig.shape[-1]
    lo, hi = float(eig.min()), float(eig.max())
    Es = np.linspace(lo - 0.1, hi + 0.1, 77)
    g, N = rule.ltm(Es), rule.ltm(Es, states=True)
    ones = np.ones((1, rule.nk, n))
    check(rule.ltm(Es, elements=ones)[:, 0], g, f"{name} ones g")
    check(rule.ltm(Es, states=True, elements="attached")[:, 0], N, f"{name} ones N")
    ge = rule.ltm(Es, elements="energy")
    assert ge.shape == (len(Es), 1)
    check(ge[:, 0], Es * g, f"{name} energy g")
    A = np.random.default_rng(2).standard_normal((3, rule.nk, n))
    top = rule.ltm(np.array([hi + 1.0]), states=True, elements=A)
    check(top[0], A.mean(axis=1).sum(axis=1), f"{name} N_A above the bands")
    band_energy = rule.ltm(np.array([hi + 1.0]), states=True, elements="energy")
    check(band_energy[0], np.array([eig.reshape(-1, n).mean(axis=0).sum()]), f"{name} band energy of the full bands")
    rule.ltm_elements(None)


# ---------------------------------------------------------------- linearity, components
def test_weighted_ltm_is_linear_and_components_are_independent(abz):
    s = svo(abz)
    rule = s.device().rule(20, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    rng = np.random.default_rng(23)
    A1, A2 = rng.standard_normal((2, rule.nk, 3))
    A = np.stack([A1, A2, 2 * A1 - 3 * A2])
    Es = np.linspace(eig.min() - 0.05, eig.max() + 0.05, 97)
    for states in (False, True):
        u = rule.ltm(Es, states=states, elements=A)
        assert u.shape == (97, 3)
        check(u[:, 2], 2 * u[:, 0] - 3 * u[:, 1], f"linearity {'N' if states else 'g'}")
        single = np.stack([rule.ltm(Es, states=states, elements=A[c:c + 1])[:, 0] for c in range(3)], axis=1)
        check(u, single, f"3 components against 3 calls {'N' if states else 'g'}")
    rule.ltm_elements(None)


# ---------------------------------------------------------------- repeatability
def test_weighted_ltm_repeatable(abz):
    s = svo(abz)
    rule = s.device().rule(20, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    rng = np.random.default_rng(11)
    rule.ltm_elements(rng.standard_normal((5, rule.nk, 3)))
    unsorted = eig.min() + (eig.max() - eig.min()) * rng.random(257)
    lin = np.linspace(eig.min(), eig.max(), 64)
    for Es in (unsorted, lin):
        for states in (False, True):
            for el in ("attached", "energy"):
                a, b = rule.ltm(Es, states=states, elements=el), rule.ltm(Es, states=states, elements=el)
                assert np.array_equal(a, b), (len(Es), states, el)
    rule.ltm_elements(None)


# ---------------------------------------------------------------- degenerate input
def test_weighted_ltm_flat_and_degenerate_bands(abz):
    """The block-diagonal H = diag(e(k), e(k), 0.25) of test_ltm_flat_and_degenerate_bands_on_device, at energies away
    from 0.25 +- ulp: at 0.25 itself, corners exactly on E with different elements, the half-open regions of the two
    codes may pick different (equally valid) sides of a jump of N_A."""
    so = orc.tb_integer(3)
    c = np.zeros((3, 3, 3, 3, 3), dtype=np.complex128)
    c[..., 0, 0] = so.c[..., 0, 0]
    c[..., 1, 1] = so.c[..., 0, 0]
    c[1, 1, 1, 2, 2] = 0.25
    s = abz.FourierSeries(c, period=1.0, first=(-1, -1, -1), ndim=3)
    rule = s.device().rule(8, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    A = np.random.default_rng(4).standard_normal((3, rule.nk, 3))
    rule.ltm_elements(A)
    sweep = np.linspace(-6.5, 6.5, 131)
    for Es in (np.array([-7.0, -1.0, 0.3, 2.0, 7.0]), sweep[np.abs(sweep - 0.25) > 1e-6]):
        g_ref, N_ref = wn.wltm(eig, on_grid(rule, A), Es)
        check(rule.ltm(Es, elements="attached"), g_ref, f"degenerate g nE={len(Es)}")
        check(rule.ltm(Es, states=True, elements="attached"), N_ref, f"degenerate N nE={len(Es)}")
    rule.ltm_elements(None)


# ---------------------------------------------------------------- Fermi level
@pytest.mark.parametrize("name,npt", [("int1", 64), ("int2", 32), ("int3", 16)])
def test_fermi_level_of_half_filled_symmetric_bands(abz, name, npt):
    """Bands symmetric about 0 on an even grid: N(0) = 1/2 to 1e-16 and N(+-1e-9) - 1/2 = +-1.4...4.3e-10 in the
    restatement, so the level lies within tol = 1e-9 of 0."""
    s = product_series(abz, MODELS[name][0]())
    rule = s.device().rule(npt, None, abz._lib.WANT_EIG)
    tol = 1e-9
    ef, nf = rule.ltm_fermi(0.5, tol)
    print(f"fermi {name} npt={npt}: E_F = {ef:.3e}, N(E_F) - 1/2 = {nf - 0.5:.3e}")
    assert abs(ef) <= tol, ef
    assert nf >= 0.5 * (1 - 1e-12)


@pytest.mark.parametrize("nstates", [0.3, 1.0, 2.5])
def test_fermi_level_svo(abz, nstates):
    s = svo(abz)
    rule = s.device().rule(20, None, abz._lib.WANT_EIG)
    tol = 1e-9
    ef, nf = rule.ltm_fermi(nstates, tol)
    N = rule.ltm(np.array([ef, ef - 2 * tol]), states=True)
    print(f"fermi svo nstates={nstates}: E_F = {ef:.12f}, N(E_F) - nstates = {N[0] - nstates:.3e}, N(E_F - 2 tol) - nstates = {N[1] - nstates:.3e}")
    assert N[0] >= nstates * (1 - 1e-12)
    assert N[1] < nstates
    assert abs(nf - N[0]) <= 1e-9 * 3
    # the Python front end on a cache
    bz = abz.load_bz(abz.FBZ(), 3.85856 * np.eye(3))
    cache = abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=20))
    ef2, _ = abz.dos.fermi_level(cache, nstates, tol)
    assert abs(ef2 - ef) <= tol


def test_fermi_level_in_a_gap(abz):
    """diag(e(k) - 8, e(k) + 8) of the 3-D model, one state: the top of the lower band to within tol.

    A search on N alone stops 2.2e-4 below the top (measured: N(top - x) = 1 - 0.09 x^3 reaches 1 - 1e-12 there, and
    in f64 it cannot tell x < 1e-5 from 0); abz_rule_ltm_fermi then narrows on g(E) == 0, which holds exactly from the
    top on."""
    so = orc.tb_integer(3)
    c = np.zeros((3, 3, 3, 2, 2), dtype=np.complex128)
    c[..., 0, 0] = so.c[..., 0, 0]
    c[..., 1, 1] = so.c[..., 0, 0]
    c[1, 1, 1, 0, 0] -= 8.0
    c[1, 1, 1, 1, 1] += 8.0
    s = abz.FourierSeries(c, period=1.0, first=(-1, -1, -1), ndim=3)
    rule = s.device().rule(16, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    top = float(eig[..., 0].max())
    assert top < float(eig[..., 1].min())
    tol = 1e-9
    ef, nf = rule.ltm_fermi(1.0, tol)
    print(f"fermi gap: E_F - top of band 1 = {ef - top:.3e}, N(E_F) - 1 = {nf - 1.0:.3e}")
    assert abs(ef - top) <= tol
    assert nf >= 1.0 - 1e-12


# ---------------------------------------------------------------- projected DOS
def test_orbital_projected_dos_sums_to_the_dos(abz):
    s = svo(abz)
    bz = abz.load_bz(abz.FBZ(), 3.85856 * np.eye(3))
    eig = ln.rule_eigenvalues(s.device().rule(20, None, abz._lib.WANT_EIG))
    Es = np.linspace(eig.min() - 0.05, eig.max() + 0.05, 64)
    plain = abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=20)).u
    sol = abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=20, elements="orbitals"))
    assert sol.u.shape == (len(Es), 3) and sol.retcode
    check(sol.u.sum(axis=1), plain, "sum of the projected DOS")
    assert np.all(sol.u >= -1e-9 * max(1.0, plain.max()))
    one = abz.dos.solve(abz.DOSProblem(s, float(Es[30]), bz), abz.LTM(npt=20, elements="orbitals")).u
    assert one.shape == (3,)
    check(one, sol.u[30], "scalar domain")
    # elements=None returns what it returned before
    assert np.array_equal(plain, s.device().rule(20, None, abz._lib.WANT_EIG).ltm(Es))


# ---------------------------------------------------------------- cache
def test_weighted_ltm_cache_follows_the_series(abz):
    """ref: test/dos.jl:113-132 in the pattern of test_ltm_cache_follows_the_series, with elements from a callable."""
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    bz = abz.load_bz(abz.FBZ(), [[2 * np.pi]])
    E = 0.3
    elements = lambda x, eig: np.stack([eig, np.cos(2 * np.pi * x[:, :1]) ** 2 + 0 * eig])
    cache = abz.dos.init(abz.DOSProblem(h, E, bz), abz.LTM(elements=elements))

    def expect(scale):
        rule = cache.cacheval
        eig = ln.rule_eigenvalues(rule)
        k = np.arange(50) / 50.0
        assert np.abs(eig[:, 0] - scale * np.cos(2 * np.pi * k)).max() <= 1e-12 * scale
        ex = rule.export(x=True, w=False, eig=True)
        return wn.wltm(eig, on_grid(rule, elements(ex["x"], ex["eig"])), [E])[0][0]

    sol1 = abz.dos.solve_(cache)
    r1 = expect(1.0)
    assert sol1.u.shape == (2,)
    check(sol1.u, r1, "cache 1")
    assert r1[0] > 0 and r1[1] > 0
    h.c *= 2
    cache.isfresh = True
    sol2 = abz.dos.solve_(cache)
    r2 = expect(2.0)
    check(sol2.u, r2, "cache 2")
    assert np.abs(r2 - r1).max() > 1e-3 and not cache.isfresh
    # a rebuild of a rule with attached elements drops them
    L = abz._lib
    rule = cache.cacheval
    rule.ltm_elements(np.ones((2, rule.nk, 1)))
    rule.rebuild()
    Es = np.array([E])
    out = np.full(2, -99.0)
    rc = L.lib().abz_rule_ltm_weighted(rule.h, L.LTM_A_ELEMENTS, Es.ctypes.data_as(L.c_f64p), 1, L.LTM_DOS, out.ctypes.data_as(L.c_f64p))
    assert rc == L.ERR_ARG and len(L.lib().abz_last_error()) > 0 and np.all(out == -99.0)
    with pytest.raises(ValueError):
        rule.ltm(Es, elements="attached")


# ---------------------------------------------------------------- memory
def test_weighted_ltm_elements_are_accounted(abz):
    L = abz._lib
    s = svo(abz)
    dev = s.device()
    ncomp, npt, n = 5, 24, 3
    A = np.random.default_rng(8).standard_normal((ncomp, npt ** 3, n))
    Es = np.linspace(11.0, 14.0, 16)

    def cycle():
        m0 = dev.ctx.mem_info()[0]
        rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
        m1 = dev.ctx.mem_info()[0]
        rule.ltm_elements(A)
        m2 = dev.ctx.mem_info()[0]
        rule.ltm(Es, elements="attached")
        rule.ltm(Es, states=True, elements="attached")
        m2b = dev.ctx.mem_info()[0]
        rule.ltm_elements(None)
        m3 = dev.ctx.mem_info()[0]
        rule.ltm_elements(A)
        rule.close()  # abz_rule_destroy with elements attached
        m4 = dev.ctx.mem_info()[0]
        return m0, m1, m2, m2b, m3, m4

    # abz_mem_info counts the whole process: rules that earlier tests dropped must be finalized before, not during, the cycle
    import gc
    gc.collect()
    gc.disable()
    try:
        cycle()  # the context's scratch buffers grow once
        m0, m1, m2, m2b, m3, m4 = cycle()
    finally:
        gc.enable()
    print(f"mem: start {m0}, rule {m1}, attached {m2} (+{m2 - m1}, elements {8 * ncomp * n * npt ** 3}), dropped {m3}, destroyed {m4}")
    assert m2 - m1 >= 8 * ncomp * n * npt ** 3
    assert m2b == m2 and m3 == m1 and m4 == m0


# ---------------------------------------------------------------- refusals
def test_weighted_ltm_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    Es = np.array([0.5, 1.5])
    out = np.full(2 * 16, -99.0)
    fermi = np.full(2, -99.0)
    pE, pout = Es.ctypes.data_as(L.c_f64p), out.ctypes.data_as(L.c_f64p)
    pef, pnf = fermi[:1].ctypes.data_as(L.c_f64p), fermi[1:].ctypes.data_as(L.c_f64p)
    A = np.ones((17, 8 ** 3, 1))
    pA = A.ctypes.data_as(L.c_f64p)

    def untouched(rc, code):
        assert rc == code, (rc, code)
        assert len(lib.abz_last_error()) > 0
        assert np.all(out == -99.0) and np.all(fermi == -99.0)  # nothing was launched or written

    def refused(h, code):
        untouched(lib.abz_rule_ltm_elements(h, pA, 1), code)
        untouched(lib.abz_rule_ltm_weighted(h, L.LTM_A_ENERGY, pE, 2, L.LTM_DOS, pout), code)
        untouched(lib.abz_rule_ltm_fermi(h, 0.5, 1e-9, pef, pnf), code)

    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, 8, cub.syms, L.WANT_EIG)
    refused(sym._h, L.ERR_UNSUPPORTED)
    assert b"not a whole periodic grid" in lib.abz_last_error()
    idx, w = abz.symptr_rule(8, 3, cub.syms)
    irr = C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, 8, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(irr)))
    refused(irr, L.ERR_UNSUPPORTED)
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, 8, 2, 6, L.WANT_EIG, C.byref(slab)))
    refused(slab, L.ERR_UNSUPPORTED)
    honly = abz.DeviceRule(dev, 8, None, L.WANT_H)
    refused(honly._h, L.ERR_ARG)
    full = abz.DeviceRule(dev, 8, None, L.WANT_EIG)
    h = full._h
    untouched(lib.abz_rule_ltm_weighted(h, L.LTM_A_ELEMENTS, pE, 2, L.LTM_DOS, pout), L.ERR_ARG)  # nothing attached
    untouched(lib.abz_rule_ltm_weighted(h, L.LTM_A_ENERGY, pE, 0, L.LTM_DOS, pout), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_weighted(h, L.LTM_A_ENERGY, None, 2, L.LTM_DOS, pout), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_weighted(h, L.LTM_A_ENERGY, pE, 2, L.LTM_DOS, None), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_weighted(h, L.LTM_A_ENERGY, pE, 2, 7, pout), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_weighted(h, 5, pE, 2, L.LTM_DOS, pout), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_elements(h, pA, 17), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_elements(h, pA, 0), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_elements(h, pA, -1), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_elements(h, None, 2), L.ERR_ARG)
    for nstates in (0.0, 1.0, -0.5, 1.5, float("nan")):  # one band: 0 < nstates < 1
        untouched(lib.abz_rule_ltm_fermi(h, nstates, 1e-9, pef, pnf), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_fermi(h, 0.5, 0.0, pef, pnf), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_fermi(h, 0.5, -1e-9, pef, pnf), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_fermi(h, 0.5, 1e-9, None, pnf), L.ERR_ARG)
    # valid calls afterwards still work; abz_rule_ltm is as it was
    assert lib.abz_rule_ltm_elements(h, pA, 2) == 0
    assert lib.abz_rule_ltm_weighted(h, L.LTM_A_ELEMENTS, pE, 2, L.LTM_DOS, pout) == 0
    ref, _ = ln.ltm(ln.rule_eigenvalues(full), Es)
    check(out[:4].reshape(2, 2), np.stack([ref, ref], axis=1), "after the refusals")
    assert np.all(out[4:] == -99.0)
    assert lib.abz_rule_ltm_fermi(h, 0.5, 1e-9, pef, None) == 0 and abs(fermi[0]) <= 1e-9 and fermi[1] == -99.0
    plain = np.zeros(2)
    assert lib.abz_rule_ltm(h, pE, 2, L.LTM_DOS, plain.ctypes.data_as(L.c_f64p)) == 0
    check(plain, ref, "abz_rule_ltm")
    assert lib.abz_rule_ltm_elements(h, None, 0) == 0
    assert lib.abz_rule_destroy(irr) == 0 and lib.abz_rule_destroy(slab) == 0
    # the Python mirror keeps the refusal of a k-sharded rule
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        r = dev.rule(8, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm(Es, elements="energy")
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_fermi(0.5)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_elements(None)
    finally:
        dev.kshard, dev.allreduce = None, None
    with pytest.raises(ValueError):
        full.ltm(Es, elements="bands")


# ---------------------------------------------------------------- profiling
def test_weighted_ltm_launches_are_profiled(abz):
    """Every launch goes through a ProfScope of ABZ_K_LTM: one per (chunk of energies, group of components), one per
    uploaded component, one for the eigenvalue bracket of the Fermi search and one per scan of it (N scans, then the
    g scan that looks for a gap above the level and the N check of what it found)."""
    L = abz._lib
    s = product_series(abz, orc.tb_integer(2))
    dev = s.device()
    rule = dev.rule(16, None, L.WANT_EIG)
    Es = np.linspace(-3, 3, 10)
    A = np.ones((3, rule.nk, 1))
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        dev.ctx.prof_reset()
        rule.ltm(Es, elements="energy")
        rule.ltm(Es, states=True, elements="energy")
        ms, launches = dev.ctx.prof_read(L.K_LTM)
        assert launches == 2 and ms > 0.0
        rule.ltm_elements(A)
        assert dev.ctx.prof_read(L.K_LTM)[1] == 2 + 3
        rule.ltm(Es, elements="attached")  # 3 components: a group of 2 and a group of 1
        assert dev.ctx.prof_read(L.K_LTM)[1] == 2 + 3 + 2
        before = dev.ctx.prof_read(L.K_LTM)[1]
        rule.ltm_fermi(0.5, 1e-9)
        scans = dev.ctx.prof_read(L.K_LTM)[1] - before - 1
        print(f"fermi search: {scans} scans")
        assert 1 <= scans <= 7  # log_511(8 / 1e-9) = 3.7: 4 or 5 N scans, one g scan for a gap above, one N check of its zero
        assert dev.ctx.prof_read(L.K_GGR)[1] == 0
    finally:
        dev.ctx.prof_enable(False)
        rule.ltm_elements(None)

"""Optimized tetrahedron method on the device (abz_rule_ltm_optimized; ltm_opt_kernel, kernels_ltm_opt.hip) against the
restatement of tests/optltm_numpy.py, which derives the projection from its definition and does not read the kernel's table.

Parity bound: the restatement is fed the rule's own exported eigenvalues and the very elements that are attached, so only
summation order, FMA contraction and the form of the product (the kernel adds sum_j P_mj (x_j - x_m) to x_m) remain; the cases
are those of test_ltm_optimized_cpu.py, whose f64 and longdouble evaluations agree to 1e-10 of the scale (seeds 101 for one band,
303 for three).  The bound is the project's LTM parity bound, |u - ref| <= 1e-9 max(1, max|ref|) (test_gpu_ltm.py)."""
import ctypes as C

import numpy as np
import pytest

import abz_oracle as orc
import ltm_numpy as ln
import optltm_numpy as on
from test_gpu_ltm import close, product_series
from test_ltm_optimized_cpu import GRIDS, SEEDS, case_coefficients, case_elements, energy_lists, sources

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def check(u, ref, what):
    assert u.shape == ref.shape and np.all(np.isfinite(u)), (what, u.shape, ref.shape)
    dev, bound = close(u, ref)
    print(f"optltm {what}: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)
    return dev / bound


def case_rule(abz, n, npt):
    c, first = case_coefficients(n)
    s = abz.FourierSeries(c, period=1.0, first=first, ndim=3)
    return s, s.device().rule(npt, None, abz._lib.WANT_EIG)


# ---------------------------------------------------------------- parity with the restatement
@pytest.mark.parametrize("n", sorted(SEEDS))
@pytest.mark.parametrize("npt", GRIDS)
def test_optimized_ltm_matches_restatement(abz, n, npt):
    s, rule = case_rule(abz, n, npt)
    eig = ln.rule_eigenvalues(rule)
    A = case_elements(n, npt)
    worst = 0.0
    for label, Es in energy_lists(eig).items():
        for states in (False, True):
            kind = "N" if states else "g"
            # the components are independent: one restatement of all 5 serves the calls with 1, 3 and 5 of them
            refs = {src: on.optltm(eig, arg, Es, states) for src, arg in sources(eig, A).items()}
            u = rule.ltm_optimized(Es, states=states)
            worst = max(worst, check(u, refs["one"][:, 0], f"n={n} npt={npt} {label} one {kind}"))
            u = rule.ltm_optimized(Es, states=states, elements="energy")
            worst = max(worst, check(u, refs["energy"], f"n={n} npt={npt} {label} energy {kind}"))
            for ncomp in (1, 3, 5):
                u = rule.ltm_optimized(Es, states=states, elements=A[:ncomp])
                worst = max(worst, check(u, refs["elements"][:, :ncomp], f"n={n} npt={npt} {label} elements {ncomp} {kind}"))
    rule.ltm_elements(None)
    print(f"optltm parity n={n} npt={npt}: worst deviation / bound = {worst:.3e}")


# ---------------------------------------------------------------- identities
@pytest.mark.parametrize("n", sorted(SEEDS))
def test_optimized_state_count_outside_the_bands(abz, n):
    s, rule = case_rule(abz, n, 7)
    eig = ln.rule_eigenvalues(rule)
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    Es = np.array([lo - 0.3 * w, hi + 0.3 * w])  # beyond every e': they leave the eigenvalues by less than 0.23 of the width
    N = rule.ltm_optimized(Es, states=True)
    assert N[0] == 0.0, N
    assert abs(N[1] - n) <= 1e-12 * n, N
    assert np.all(rule.ltm_optimized(Es) == 0.0)
    # A = 1 as attached elements
    mid = np.linspace(lo, hi, 33)
    ones = np.ones((1, rule.nk, n))
    for states in (False, True):
        a, b = rule.ltm_optimized(mid, states=states, elements=ones)[:, 0], rule.ltm_optimized(mid, states=states)
        dev = np.abs(a - b).max()
        print(f"n={n} elements == 1 against one, {'N' if states else 'g'}: {dev:.2e}")
        assert dev <= 1e-12 * max(1.0, np.abs(b).max())
    rule.ltm_elements(None)


def test_optimized_flat_band(abz):
    c = np.zeros((3, 3, 3, 1, 1), dtype=np.complex128)
    c[1, 1, 1, 0, 0] = 0.25
    s = abz.FourierSeries(c, period=1.0, first=(-1, -1, -1), ndim=3)
    rule = s.device().rule(6, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    v = float(eig.reshape(-1)[0])
    assert np.all(eig == v) and abs(v - 0.25) <= 1e-15
    Es = np.array([v - 1.0, np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf), v + 1.0])
    assert np.all(rule.ltm_optimized(Es) == 0.0)
    N = rule.ltm_optimized(Es, states=True)
    assert np.all(N[:2] == 0.0) and np.abs(N[2:] - 1.0).max() <= 1e-15, N
    NE = rule.ltm_optimized(Es, states=True, elements="energy")[:, 0]
    assert np.all(NE[:2] == 0.0) and np.abs(NE[2:] - v).max() <= 1e-15, NE


def test_optimized_ltm_repeatable_and_takes_any_order(abz):
    s, rule = case_rule(abz, 3, 8)
    eig = ln.rule_eigenvalues(rule)
    rng = np.random.default_rng(11)
    rule.ltm_elements(case_elements(3, 8))
    unsorted = eig.min() + (eig.max() - eig.min()) * rng.random(257)
    lin = np.linspace(eig.min(), eig.max(), 64)
    for Es in (unsorted, lin):
        for states in (False, True):
            for el in (None, "energy", "attached"):
                a, b = rule.ltm_optimized(Es, states=states, elements=el), rule.ltm_optimized(Es, states=states, elements=el)
                assert np.array_equal(a, b), (len(Es), states, el)
    # the energy list is abz_rule_ltm_weighted's: any order, results in the caller's order
    order = np.argsort(unsorted)
    for states in (False, True):
        a = rule.ltm_optimized(unsorted, states=states, elements="attached")
        b = rule.ltm_optimized(unsorted[order], states=states, elements="attached")
        assert np.array_equal(a[order], b)
    rule.ltm_elements(None)


def test_optimized_ltm_on_an_unfolded_rule(abz):
    """the cubic-symmetric 3-d model: eigenvalues gathered from the irreducible nodes against the full grid's own"""
    L = abz._lib
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    full = dev.rule(8, None, L.WANT_EIG)
    unf = dev.rule(8, cub.syms, L.WANT_EIG).unfold()
    eig = ln.rule_eigenvalues(full)
    Es = np.linspace(eig.min() - 0.5, eig.max() + 0.5, 41)
    for states in (False, True):
        for el in (None, "energy"):
            check(unf.ltm_optimized(Es, states=states, elements=el), full.ltm_optimized(Es, states=states, elements=el),
                  f"unfolded {'N' if states else 'g'} {el}")
    check(full.ltm_optimized(Es, states=True), on.optltm(eig, None, Es, True)[:, 0], "int3 N against the restatement")


def test_optimized_ltm_is_not_the_plain_scan(abz):
    s, rule = case_rule(abz, 3, 8)
    eig = ln.rule_eigenvalues(rule)
    Es = energy_lists(eig)["equispaced"]
    for states in (False, True):
        diff = np.abs(rule.ltm_optimized(Es, states=states) - rule.ltm(Es, states=states)).max()
        print(f"optimized against plain, {'N' if states else 'g'}: {diff:.3e}")
        assert diff > 1e-4


# ---------------------------------------------------------------- refusals
def test_optimized_ltm_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s, full = case_rule(abz, 1, 8)
    dev = s.device()
    Es = np.array([0.5, 1.5])
    out = np.full(2 * 16, -99.0)
    pE, pout = Es.ctypes.data_as(L.c_f64p), out.ctypes.data_as(L.c_f64p)

    def untouched(rc, code):
        assert rc == code, (rc, code)
        assert len(lib.abz_last_error()) > 0
        assert np.all(out == -99.0)  # nothing was launched or written

    def refused(h, code):
        for source in (L.LTM_A_ONE, L.LTM_A_ENERGY, L.LTM_A_ELEMENTS):
            for what in (L.LTM_DOS, L.LTM_STATES):
                untouched(lib.abz_rule_ltm_optimized(h, source, pE, 2, what, pout), code)

    # d = 2
    s2 = product_series(abz, orc.tb_integer(2))
    flat = abz.DeviceRule(s2.device(), 8, None, L.WANT_EIG)
    refused(flat._h, L.ERR_UNSUPPORTED)
    assert b"d = 2" in lib.abz_last_error()
    with pytest.raises(NotImplementedError, match="d = 3"):
        flat.ltm_optimized(Es)
    plain2 = flat.ltm(Es)
    # a slab, without and with its halo plane
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, 8, 2, 6, L.WANT_EIG, C.byref(slab)))
    refused(slab, L.ERR_UNSUPPORTED)
    L.check(lib.abz_rule_ltm_halo(slab))
    refused(slab, L.ERR_UNSUPPORTED)
    partial = np.zeros(2)
    assert lib.abz_rule_ltm(slab, pE, 2, L.LTM_DOS, partial.ctypes.data_as(L.c_f64p)) == 0  # the slab still serves the linear scan
    # irreducible nodes
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    idx, w = abz.symptr_rule(8, 3, cub.syms)
    irr = C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, 8, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(irr)))
    refused(irr, L.ERR_UNSUPPORTED)
    assert b"not a whole periodic grid" in lib.abz_last_error()
    # a rule without eigenvalues
    honly = abz.DeviceRule(dev, 8, None, L.WANT_H)
    refused(honly._h, L.ERR_ARG)
    # the full grid: arguments
    h = full._h
    plain = full.ltm(Es)
    for source in (L.LTM_A_ONE, L.LTM_A_ENERGY):
        untouched(lib.abz_rule_ltm_optimized(h, source, pE, 2, L.LTM_STATES_CORRECTED, pout), L.ERR_ARG)
        assert b"replaces" in lib.abz_last_error()
        untouched(lib.abz_rule_ltm_optimized(h, source, pE, 2, 7, pout), L.ERR_ARG)
        untouched(lib.abz_rule_ltm_optimized(h, source, None, 2, L.LTM_DOS, pout), L.ERR_ARG)
        untouched(lib.abz_rule_ltm_optimized(h, source, pE, 2, L.LTM_DOS, None), L.ERR_ARG)
        untouched(lib.abz_rule_ltm_optimized(h, source, pE, 0, L.LTM_DOS, pout), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_optimized(h, 5, pE, 2, L.LTM_DOS, pout), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_optimized(h, L.LTM_A_ELEMENTS, pE, 2, L.LTM_DOS, pout), L.ERR_ARG)  # nothing attached
    assert b"no matrix elements" in lib.abz_last_error()
    with pytest.raises(ValueError):
        full.ltm_optimized(Es, elements="attached")
    with pytest.raises(ValueError):
        full.ltm_optimized(Es, elements="bands")
    # the rules are as they were: the linear scans return the same bits, a valid call works and writes its own results only
    assert np.array_equal(full.ltm(Es), plain) and np.array_equal(flat.ltm(Es), plain2)
    assert lib.abz_rule_ltm_optimized(h, L.LTM_A_ONE, pE, 2, L.LTM_STATES, pout) == 0
    check(out[:2], on.optltm(ln.rule_eigenvalues(full), None, Es, True)[:, 0], "after the refusals")
    assert np.all(out[2:] == -99.0)
    assert lib.abz_rule_destroy(irr) == 0 and lib.abz_rule_destroy(slab) == 0
    # the Python mirror refuses a k-sharded rule before it asks the library
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        r = dev.rule(8, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_optimized(Es)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_fermi_optimized(0.5)
        bz = abz.load_bz(abz.FBZ(), np.eye(3))
        with pytest.raises(NotImplementedError, match="k-sharded"):
            abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=8, optimized=True))
    finally:
        dev.kshard, dev.allreduce = None, None


def test_optimized_ltm_launches_are_profiled(abz):
    L = abz._lib
    s, rule = case_rule(abz, 3, 8)
    dev = s.device()
    Es = np.linspace(-3, 3, 10)
    rule.ltm_elements(case_elements(3, 8)[:3])
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        dev.ctx.prof_reset()
        rule.ltm_optimized(Es)
        rule.ltm_optimized(Es, states=True, elements="energy")
        ms, launches = dev.ctx.prof_read(L.K_LTM)
        assert launches == 2 and ms > 0.0
        rule.ltm_optimized(Es, elements="attached")  # 3 components: a group of 2 and a group of 1
        assert dev.ctx.prof_read(L.K_LTM)[1] == 2 + 2
    finally:
        dev.ctx.prof_enable(False)
        rule.ltm_elements(None)


# ---------------------------------------------------------------- the Python front end
def test_optimized_ltm_problem_solve_equals_the_rule_call(abz):
    L = abz._lib
    c, first = case_coefficients(3)
    s = abz.FourierSeries(c, period=1.0, first=first, ndim=3)
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    rule = s.device().rule(8, None, L.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    Es = np.linspace(eig.min(), eig.max(), 17)
    sol = abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=8, optimized=True))
    assert sol.retcode and np.array_equal(sol.u, rule.ltm_optimized(Es))
    sol = abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=8, optimized=True, cumulative=True, elements="energy"))
    assert sol.u.shape == (17, 1) and np.array_equal(sol.u, rule.ltm_optimized(Es, states=True, elements="energy"))
    f = lambda x, e: np.stack([e, np.cos(2 * np.pi * x[:, :1]) + 0 * e])
    sol = abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=8, optimized=True, elements=f))
    ex = rule.export(x=True, w=False, eig=True)
    assert sol.u.shape == (17, 2) and np.array_equal(sol.u, rule.ltm_optimized(Es, elements=f(ex["x"], ex["eig"])))
    one = abz.dos.solve(abz.DOSProblem(s, float(Es[5]), bz), abz.LTM(npt=8, optimized=True)).u
    assert one == rule.ltm_optimized(Es[5:6])[0]
    rule.ltm_elements(None)
    # optimized=False returns what it returned before
    assert np.array_equal(abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=8)).u, rule.ltm(Es))
    # symmetric=True: the unfolded rule of the cubic model
    sc = product_series(abz, orc.tb_integer(3))
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    Ec = np.linspace(-5.5, 5.5, 12)
    a = abz.dos.solve(abz.DOSProblem(sc, Ec, cub), abz.LTM(npt=8, optimized=True, symmetric=True)).u
    check(a, sc.device().rule(8, None, L.WANT_EIG).ltm_optimized(Ec), "LTM(optimized, symmetric)")


def test_optimized_fermi_level_of_half_filled_symmetric_bands(abz):
    """The 3-d case of test_fermi_level_of_half_filled_symmetric_bands: e(k + (1/2, 1/2, 1/2)) = -e(k) on an even grid carries every
    simplex, stencil included, to one with e' -> -e', so N(0) = 1/2 for the optimized rule too and the level lies within tol of 0."""
    from test_ltm_cpu import MODELS
    s = product_series(abz, MODELS["int3"][0]())
    rule = s.device().rule(16, None, abz._lib.WANT_EIG)
    tol = 1e-9
    ef, nf = rule.ltm_fermi_optimized(0.5, tol)
    print(f"optimized fermi int3 npt=16: E_F = {ef:.3e}, N(E_F) - 1/2 = {nf - 0.5:.3e}")
    assert abs(ef) <= tol, ef
    assert nf >= 0.5 * (1 - 1e-12)
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    cache = abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=16))
    ef2, _ = abz.dos.fermi_level(cache, 0.5, tol, optimized=True)
    assert abs(ef2) <= tol
    assert abz.dos.fermi_level(cache, 0.5, tol) == rule.ltm_fermi(0.5, tol)  # the default stays the linear rule's level


def test_optimized_fermi_level_at_a_generic_filling(abz):
    """Three random bands at npt = 8, 1.3 states: g is about 3 / width << 1 there, so an interval of tol holds less than tol states."""
    s, rule = case_rule(abz, 3, 8)
    tol = 1e-9
    nstates = 1.3
    ef, nf = rule.ltm_fermi_optimized(nstates, tol)
    N = rule.ltm_optimized(np.array([ef, ef - 2 * tol]), states=True)
    print(f"optimized fermi nstates={nstates}: E_F = {ef:.12f}, N(E_F) - nstates = {N[0] - nstates:.3e}, N(E_F - 2 tol) - nstates = {N[1] - nstates:.3e}")
    assert abs(N[0] - nstates) <= 3 * tol
    assert N[0] >= nstates * (1 - 1e-12) and N[1] < nstates
    assert abs(nf - N[0]) <= 3 * tol  # (the search's scan sums its steps over 512 energies, this one over 2)
    plain = rule.ltm_fermi(nstates, tol)[0]
    assert 1e-6 < abs(plain - ef) < 0.5  # another rule, the same band structure
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    cache = abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=8, optimized=True))
    assert abz.dos.fermi_level(cache, nstates, tol) == (ef, nf)
    eb, ef3 = abz.dos.band_energy(cache, nstates, tol)
    assert ef3 == ef and eb == rule.ltm_optimized(np.array([ef]), states=True, elements="energy")[0, 0]

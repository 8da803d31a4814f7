"""Linear tetrahedron method on the device (abz_rule_ltm, kernels_ltm.hip) against the numpy restatement of
tests/ltm_numpy.py and the reference's exact DOS formulas.

Parity bound: the restatement is fed the rule's own exported eigenvalues, so only summation order and FMA contraction
remain; the bound is the GGR scan's, |u - ref| <= 1e-9 max(1, max|ref|) (test_gpu_parity.py::test_ggr_matches_oracle_and_exact).
"""
import ctypes as C
import os

import numpy as np
import pytest

import abz_oracle as orc
import ltm_numpy as ln
from test_ltm_cpu import MODELS, reference_energies

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def product_series(abz, so):
    return abz.FourierSeries(so.c, period=1.0, first=so.first, ndim=so.d)


def close(u, ref):
    """(deviation, bound) of the parity check."""
    return np.abs(np.asarray(u) - np.asarray(ref)).max(), 1e-9 * max(1.0, np.abs(ref).max())


def check_parity(rule, Es, eig=None, what="", both=True):
    eig = ln.rule_eigenvalues(rule) if eig is None else eig
    g_ref, N_ref = ln.ltm(eig, Es)
    worst = 0.0
    for states, ref in ((False, g_ref), (True, N_ref)) if both else ((False, g_ref),):
        u = rule.ltm(Es, states=states)
        assert u.shape == ref.shape and np.all(np.isfinite(u)), (what, states)
        dev, bound = close(u, ref)
        print(f"ltm parity {what} nE={len(Es)} {'N' if states else 'g'}: max dev {dev:.3e} (bound {bound:.1e})")
        assert dev <= bound, (what, states, dev, bound)
        worst = max(worst, dev / bound)
    return worst


# ---------------------------------------------------------------- 5. the reference's DOS test with LTM in the tuple
@pytest.mark.parametrize("name", ["int1", "int2", "graphene", "int3"])
def test_ltm_vs_exact_dos_all_zone_kinds(abz, name):
    """ref: test/dos.jl:88-111, `for alg in (GGR(; npt=200), LTM(; npt=200))`: |u - exact| < 1e-2 at the reference's ten
    energies, for every zone kind; all kinds run the full grid, so their values are bit-identical."""
    make, exact, B = MODELS[name]
    so = make()
    Es = reference_energies(B)
    kinds = [abz.FBZ(), abz.InversionSymIBZ(), abz.CubicSymIBZ()]
    got = []
    for kind in kinds:
        s = product_series(abz, so)
        bz = abz.load_bz(kind, np.eye(so.d))
        cache = abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=200))
        us = []
        for e in Es:
            cache.domain = e
            sol = abz.dos.solve_(cache)
            assert isinstance(sol.u, float) and sol.retcode
            us.append(sol.u)
        err = max(abs(u - exact(e)) for u, e in zip(us, Es))
        print(f"ltm vs exact {name} {type(kind).__name__}: max err {err:.3e}")
        assert err < 1e-2, (name, type(kind).__name__, us)
        got.append(np.array(us))
    for other in got[1:]:
        assert np.array_equal(got[0], other)


# ---------------------------------------------------------------- 6. parity with the restatement
def energy_lists(eig, rng):
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    gamma = eig[(0,) * (eig.ndim - 1)]  # eigenvalues of the Gamma point (node 0)
    return {
        "one": np.array([lo + 0.37 * w]),
        "seven": lo + w * np.array([0.7, 0.1, 0.5, 0.3, 0.5, 0.95, -0.1]),  # unsorted, one duplicate, one below the bands
        "linspace300": np.linspace(lo - 0.05 * w, hi + 0.05 * w, 300),
        "many1500": lo - 0.05 * w + 1.1 * w * rng.random(1500),  # unsorted, two chunks (three for N)
        "edges": np.array([gamma[0], gamma[-1], gamma[len(gamma) // 2], lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf),
                           np.nextafter(hi, -np.inf)]),
    }


def parity_cases():
    return ["int1", "int2", "graphene", "int3", "svo", "syn6", "syn16", "syn17", "syn33"]


def make_case(abz, name):
    if name in MODELS:
        so = MODELS[name][0]()
        return product_series(abz, so), {"int1": 101, "int2": 40, "graphene": 36, "int3": 24}[name]
    if name == "svo":
        return abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz")), 20
    n = int(name[3:])
    return product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7)), 12  # one case per eigenvalue-kernel family


@pytest.mark.parametrize("name", parity_cases())
def test_ltm_matches_restatement(abz, name):
    s, npt = make_case(abz, name)
    rule = s.device().rule(npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    assert np.all(np.diff(eig, axis=-1) >= 0.0)  # ascending per node
    rng = np.random.default_rng(5)
    worst = 0.0
    for label, Es in energy_lists(eig, rng).items():
        worst = max(worst, check_parity(rule, Es, eig, what=f"{name} npt={npt} {label}"))
    print(f"ltm parity {name}: worst deviation / bound = {worst:.3e}")


# ---------------------------------------------------------------- 7. degenerate input on the device
def test_ltm_flat_and_degenerate_bands_on_device(abz):
    """Block-diagonal H = diag(e(k), e(k), 0.25), npt 8: two exactly degenerate bands and a flat one crossing them."""
    so = orc.tb_integer(3)
    c = np.zeros((3, 3, 3, 3, 3), dtype=np.complex128)
    c[..., 0, 0] = so.c[..., 0, 0]
    c[..., 1, 1] = so.c[..., 0, 0]
    c[1, 1, 1, 2, 2] = 0.25
    s = abz.FourierSeries(c, period=1.0, first=(-1, -1, -1), ndim=3)
    rule = s.device().rule(8, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    Es = np.array([-7.0, -1.0, np.nextafter(0.25, -1.0), 0.25, np.nextafter(0.25, 1.0), 0.3, 2.0, 7.0])
    check_parity(rule, Es, eig, what="degenerate")
    check_parity(rule, np.linspace(-6.5, 6.5, 131), eig, what="degenerate sweep")
    N = rule.ltm(Es, states=True)
    assert N[0] == 0.0 and abs(N[-1] - 3.0) <= 3e-12 and np.all(np.diff(N) >= 0.0)


# ---------------------------------------------------------------- 8. state count
def test_ltm_state_count_svo(abz):
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    bz = abz.load_bz(abz.FBZ(), 3.85856 * np.eye(3))
    alg = abz.LTM(npt=20, cumulative=True)
    N = abz.dos.solve(abz.DOSProblem(s, [0.0, 100.0], bz), alg).u
    assert N[0] == 0.0
    assert abs(N[1] - 3.0) <= 1e-12, N[1]
    eig = ln.rule_eigenvalues(s.device().rule(20, None, abz._lib.WANT_EIG))
    sweep = np.linspace(eig.min() - 0.1, eig.max() + 0.1, 256)
    Ns = abz.dos.solve(abz.DOSProblem(s, sweep, bz), alg).u
    assert Ns[0] == 0.0 and abs(Ns[-1] - 3.0) <= 1e-12 and np.all(np.diff(Ns) >= 0.0)
    # the scalar domain
    one = abz.dos.solve(abz.DOSProblem(s, float(sweep[100]), bz), alg).u
    assert isinstance(one, float) and abs(one - Ns[100]) <= 1e-9 * 3


# ---------------------------------------------------------------- 9. repeatability
def test_ltm_repeatable(abz):
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    rule = s.device().rule(20, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    rng = np.random.default_rng(11)
    Es = eig.min() + (eig.max() - eig.min()) * rng.random(257)
    for states in (False, True):
        a, b = rule.ltm(Es, states=states), rule.ltm(Es, states=states)
        assert np.array_equal(a, b)
        for i in (0, 100, 256):
            alone = rule.ltm(Es[i:i + 1], states=states)
            dev, bound = close(alone, a[i:i + 1])
            assert dev <= 1e-9 * max(1.0, np.abs(a).max()), (states, i, dev)
    lin = np.linspace(eig.min(), eig.max(), 64)
    assert np.array_equal(rule.ltm(lin), rule.ltm(lin))


# ---------------------------------------------------------------- 10. cache
def test_ltm_cache_follows_the_series(abz):
    """ref: test/dos.jl:113-132 for LTM: mutate the coefficients in place and set isfresh, then assign a new H."""
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    bz = abz.load_bz(abz.FBZ(), [[2 * np.pi]])
    E = 0.3
    cache = abz.dos.init(abz.DOSProblem(h, E, bz), abz.LTM())
    k = np.arange(50) / 50.0

    def expect(scale):
        band = (scale * np.cos(2 * np.pi * k))[:, None]
        eig = ln.rule_eigenvalues(cache.cacheval)
        assert np.abs(eig - band).max() <= 1e-12 * scale
        return ln.ltm(eig, [E])[0][0]

    sol1 = abz.dos.solve_(cache)
    r1 = expect(1.0)
    assert r1 > 0 and abs(sol1.u - r1) <= 1e-9 * max(1.0, r1)
    h.c *= 2
    cache.isfresh = True
    sol2 = abz.dos.solve_(cache)
    r2 = expect(2.0)
    assert abs(sol2.u - r2) <= 1e-9 * max(1.0, r2) and abs(r2 - r1) > 1e-3
    cache.H = abz.FourierSeries(2 * h.c, period=1.0, offset=-2)
    assert cache.isfresh
    sol3 = abz.dos.solve_(cache)
    r3 = expect(4.0)
    assert abs(sol3.u - r3) <= 1e-9 * max(1.0, r3) and abs(r3 - r2) > 1e-3
    assert not cache.isfresh


# ---------------------------------------------------------------- 11. refusals
def test_ltm_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    Es = np.array([0.5, 1.5])
    out = np.full(2, -99.0)
    pE, pout = Es.ctypes.data_as(L.c_f64p), out.ctypes.data_as(L.c_f64p)

    def refused(h, code, nE=2, what=L.LTM_DOS, E=pE, o=pout):
        assert lib.abz_rule_ltm(h, E, nE, what, o) == code
        assert len(lib.abz_last_error()) > 0
        assert np.all(out == -99.0)  # nothing was launched or written

    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, 8, cub.syms, L.WANT_EIG)  # built with a symmetry set on the device
    refused(sym._h, L.ERR_UNSUPPORTED)
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
    refused(full._h, L.ERR_ARG, nE=0)
    refused(full._h, L.ERR_ARG, what=7)
    refused(full._h, L.ERR_ARG, E=None)
    refused(full._h, L.ERR_ARG, o=None)
    # a valid call afterwards still works
    assert lib.abz_rule_ltm(full._h, pE, 2, L.LTM_DOS, pout) == 0
    ref, _ = ln.ltm(ln.rule_eigenvalues(full), Es)
    dev_, bound = close(out, ref)
    assert dev_ <= bound
    assert lib.abz_rule_destroy(irr) == 0 and lib.abz_rule_destroy(slab) == 0
    # the Python mirror: a k-sharded (slab) rule names the limit
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        with pytest.raises(NotImplementedError, match="halo"):
            dev.rule(8, None, L.WANT_EIG).ltm(Es)
    finally:
        dev.kshard, dev.allreduce = None, None
    with pytest.raises(ValueError):
        abz.dos.solve(abz.DOSProblem(s, "band", abz.load_bz(abz.FBZ(), np.eye(3))), abz.LTM(npt=8))


def test_ltm_launches_are_profiled(abz):
    """Every launch goes through a ProfScope of ABZ_K_LTM."""
    L = abz._lib
    s = product_series(abz, orc.tb_integer(2))
    dev = s.device()
    rule = dev.rule(16, None, L.WANT_EIG)
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        dev.ctx.prof_reset()
        rule.ltm(np.linspace(-3, 3, 10))
        rule.ltm(np.linspace(-3, 3, 10), states=True)
        ms, launches = dev.ctx.prof_read(L.K_LTM)
        assert launches == 2 and ms > 0.0
        assert dev.ctx.prof_read(L.K_GGR)[1] == 0
    finally:
        dev.ctx.prof_enable(False)

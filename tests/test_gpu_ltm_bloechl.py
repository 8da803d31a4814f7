"""Bloechl's curvature correction of the weighted state sums on the device (ABZ_LTM_STATES_CORRECTED of
abz_rule_ltm_weighted; ltm_window_kernel<D, true, SLAB, LtmElems<NC, true>> of kernels_ltm.hip) against the numpy restatements:
N_A of tests/wltm_numpy.py plus the correction of tests/bloechl_numpy.py, both fed the rule's own exported eigenvalues
and the very elements that are attached.

Parity bound: |u - ref| <= 1e-9 max(1, max|ref|), the project's LTM bound (test_gpu_ltm.py); a difference of two device
results against the correction alone gets twice that."""
import ctypes as C
import os

import numpy as np
import pytest

import abz_oracle as orc
import bloechl_numpy as bn
import ltm_numpy as ln
import wltm_numpy as wn
from test_gpu_ltm import GOLD, close, product_series

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def cosine_series(abz, d, t=(1.0, 1.0, 1.0), diag=0.0):
    """-2 sum_j t_j cos 2 pi x_j + diag cos 2 pi (x_1 + x_2): the band bn.cosine_band tabulates"""
    c = np.zeros((3,) * d + (1, 1), dtype=np.complex128)
    for j in range(d):
        for side in (0, 2):
            idx = [1] * d
            idx[j] = side
            c[tuple(idx) + (0, 0)] = -t[j]
    if diag:
        for side in (0, 2):
            c[(side, side) + (1,) * (d - 2) + (0, 0)] = 0.5 * diag
    return abz.FourierSeries(c, period=1.0, first=(-1,) * d, ndim=d)


MODEL_A = dict(d=3)
MODEL_B = dict(d=3, t=(1.0, 0.8, 0.6), diag=0.5)

CASES = {
    "cos1-37": (lambda abz: cosine_series(abz, 1), 37),
    "cos2-13": (lambda abz: cosine_series(abz, 2, (1.0, 0.7), 0.5), 13),
    "cosA-5": (lambda abz: cosine_series(abz, **MODEL_A), 5),    # fewer than 256 cells: one partial pass
    "cosA-12": (lambda abz: cosine_series(abz, **MODEL_A), 12),  # 6.75 passes
    "cosB-5": (lambda abz: cosine_series(abz, **MODEL_B), 5),
    "cosB-12": (lambda abz: cosine_series(abz, **MODEL_B), 12),
    "svo-8": (lambda abz: abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz")), 8),
    "syn6-6": (lambda abz: product_series(abz, orc.synthetic_wannier(6, rmax=2, seed=7)), 6),
}


def make_rule(abz, name):
    make, npt = CASES[name]
    return make(abz).device().rule(npt, None, abz._lib.WANT_EIG)


def energy_lists(eig):
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    gamma = eig[(0,) * (eig.ndim - 1)]  # eigenvalues of the Gamma point (node 0)
    return {
        "one": np.array([lo + 0.37 * w]),  # few cells hold it: the queue path
        "seven": lo + w * np.array([0.7, 0.1, 0.5, 0.3, 0.5, 0.95, -0.1]),  # unsorted, one duplicate, one below the bands
        "linspace300": np.linspace(lo - 0.05 * w, hi + 0.05 * w, 300),  # the direct walk; two chunks at NC = 4 (155 each)
        "edges": np.array([gamma[0], gamma[-1], gamma[len(gamma) // 2], lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf),
                           np.nextafter(hi, -np.inf)]),
    }


def on_grid(rule, A):
    d = rule.dev.s.d
    return A.reshape((A.shape[0],) + (rule.npt,) * d + (A.shape[-1],))


def check(u, ref, what, factor=1.0, scale=None):
    assert u.shape == ref.shape and np.all(np.isfinite(u)), (what, u.shape, ref.shape)
    dev = np.abs(u - ref).max()
    bound = factor * close(ref if scale is None else scale, ref if scale is None else scale)[1]  # factor x 1e-9 max(1, max|scale|)
    print(f"bloechl {what}: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)
    return dev / bound


def references(rule):
    """Per energy list: (N_A, correction) of the restatements for 16 random components (seed 5) and, last column, A = e."""
    eig = ln.rule_eigenvalues(rule)
    n = eig.shape[-1]
    A = np.random.default_rng(5).standard_normal((16, rule.nk, n))
    allA = np.concatenate([on_grid(rule, A), eig[None]])
    simplices = bn.sorted_simplices(eig, allA)
    lists = energy_lists(eig)
    return A, lists, {label: (wn.wltm(eig, allA, Es)[1], bn.correction_from(simplices, Es)) for label, Es in lists.items()}


# ---------------------------------------------------------------- 1. parity, 2. differences
@pytest.mark.parametrize("name", list(CASES))
def test_corrected_ltm_matches_restatement(abz, name):
    rule = make_rule(abz, name)
    A, lists, refs = references(rule)
    worst = 0.0
    for ncomp in (1, 3, 16):  # groups of 1 | 2 + 1 | 4 x 4 components
        rule.ltm_elements(A[:ncomp])
        for label, Es in lists.items():
            N_ref, c_ref = refs[label]
            u = rule.ltm(Es, states=True, elements="attached", correction=True)
            ref = (N_ref + c_ref)[:, :ncomp]
            worst = max(worst, check(u, ref, f"{name} {label} ncomp={ncomp} N_A^corr"))
            plain = rule.ltm(Es, states=True, elements="attached")
            check(u - plain, c_ref[:, :ncomp], f"{name} {label} ncomp={ncomp} corrected - plain", factor=2.0, scale=ref)
    rule.ltm_elements(None)
    for label, Es in lists.items():
        N_ref, c_ref = refs[label]
        u = rule.ltm(Es, states=True, elements="energy", correction=True)
        ref = (N_ref + c_ref)[:, 16:]
        worst = max(worst, check(u, ref, f"{name} {label} energy N_e^corr"))
        check(u - rule.ltm(Es, states=True, elements="energy"), c_ref[:, 16:], f"{name} {label} energy corrected - plain", factor=2.0,
              scale=ref)
    print(f"bloechl parity {name}: worst deviation / bound = {worst:.3e}")


@pytest.mark.parametrize("name", ["cos1-37", "cos2-13", "cosB-12", "svo-8"])
def test_correction_of_unit_elements_is_zero(abz, name):
    rule = make_rule(abz, name)
    eig = ln.rule_eigenvalues(rule)
    rule.ltm_elements(np.ones((1, rule.nk, eig.shape[-1])))
    for label, Es in energy_lists(eig).items():
        plain = rule.ltm(Es, states=True, elements="attached")
        check(rule.ltm(Es, states=True, elements="attached", correction=True), plain, f"{name} {label} A = 1")
        check(plain[:, 0], rule.ltm(Es, states=True), f"{name} {label} A = 1 against the unweighted count")
    rule.ltm_elements(None)


# ---------------------------------------------------------------- 3. what the correction is for
@pytest.fixture(scope="module")
def reference_band_energy():
    """the corrected restatement at 64^3, filling 0.30 of -2 (cos k1 + cos k2 + cos k3)"""
    return bn.band_energy(bn.cosine_band(64), 0.30)[0]


@pytest.mark.parametrize("npt", [12, 16])
def test_corrected_band_energy_converges_faster_on_the_device(abz, npt, reference_band_energy):
    """The condition of test_ltm_bloechl_cpu.py::test_corrected_band_energy_converges_faster with the device's Fermi level
    and scans: the corrected error is at most a fifth of the plain one."""
    s = cosine_series(abz, **MODEL_A)
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    cache = abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=npt))
    ef, _ = cache.cacheval.ltm_fermi(0.30, 1e-10)
    Ec, ef_c = abz.dos.band_energy(cache, 0.30)
    Ep, ef_p = abz.dos.band_energy(cache, 0.30, correction=False)
    assert ef_c == ef and ef_p == ef
    assert Ep == cache.cacheval.ltm(np.array([ef]), states=True, elements="energy")[0, 0]
    plain, corr = Ep - reference_band_energy, Ec - reference_band_energy
    print(f"device npt={npt}: E_F = {ef:.10f}, band-energy error plain {plain:+.3e}, corrected {corr:+.3e}, ratio {abs(plain) / abs(corr):.1f}")
    assert abs(corr) <= abs(plain) / 5.0
    # from a problem instead of a cache: LTM() at its default npt = 50.  The plain error falls like 1 / npt^2 from 4.9e-3 at
    # npt = 24 to 1.1e-3 at 50; the corrected value lies below that
    Eb, _ = abz.dos.band_energy(abz.DOSProblem(s, 0.0, bz), 0.30)
    assert abs(Eb - reference_band_energy) <= 1.1e-3


# ---------------------------------------------------------------- 4. unfolded rule, the routes of the front end
def test_corrected_ltm_on_an_unfolded_rule(abz):
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    cub = abz.load_bz(abz.CubicSymIBZ(), 3.85856 * np.eye(3))
    full = s.device().rule(8, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(full)
    Es = np.linspace(eig.min() - 0.05, eig.max() + 0.05, 61)
    alg = abz.LTM(npt=8, symmetric=True, cumulative=True, elements="energy", correction=True)
    cache = abz.dos.init(abz.DOSProblem(s, Es, cub), alg)
    assert isinstance(cache.cacheval, abz.UnfoldedRule)
    u = abz.dos.solve_(cache).u
    ref = full.ltm(Es, states=True, elements="energy", correction=True)
    check(u, ref, "unfolded against the full grid")
    assert np.abs(ref - full.ltm(Es, states=True, elements="energy")).max() > 1e-4  # the correction is there


def test_corrected_ltm_front_end_routes(abz):
    """LTM(correction=True) on every route of the cache: corrected minus plain is the restatement's correction of the
    elements the rule then holds."""
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    bz = abz.load_bz(abz.FBZ(), 3.85856 * np.eye(3))
    f = lambda x, eig: np.stack([eig, np.cos(2 * np.pi * x[:, :1]) ** 2 + 0 * eig])
    routes = {
        "energy": dict(elements="energy"),
        "callable": dict(elements=f),
        "orbitals host": dict(elements="orbitals"),
        "orbitals device": dict(elements="orbitals", eigenvectors="device"),
    }
    for label, kw in routes.items():
        sols = {}
        for correction in (False, True):
            cache = abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=8, cumulative=True, correction=correction, **kw))
            rule = cache.cacheval
            eig = ln.rule_eigenvalues(rule)
            cache.domain = np.linspace(eig.min() + 0.1, eig.max() - 0.1, 9)
            sols[correction] = abz.dos.solve_(cache).u
        A = eig[None] if label == "energy" else on_grid(rule, rule.ltm_elements_export())
        c_ref = bn.correction(eig, A, cache.domain)
        assert np.abs(c_ref).max() > 1e-5
        check(sols[True] - sols[False], c_ref, f"route {label}", factor=2.0, scale=sols[True])
        rule.ltm_elements(None)
    rule = s.device().rule(8, None, abz._lib.WANT_EIG)
    with pytest.raises(ValueError, match="states"):
        rule.ltm(cache.domain, elements="energy", correction=True)
    with pytest.raises(ValueError, match="elements"):
        rule.ltm(cache.domain, states=True, correction=True)


# ---------------------------------------------------------------- 5. repeatability, 6. launches
def test_corrected_ltm_repeatable_and_launch_counts(abz):
    L = abz._lib
    rule = make_rule(abz, "cosB-12")
    eig = ln.rule_eigenvalues(rule)
    rng = np.random.default_rng(11)
    rule.ltm_elements(rng.standard_normal((7, rule.nk, 1)))  # groups of 4, 2 and 1
    unsorted = eig.min() + (eig.max() - eig.min()) * rng.random(257)
    dev = rule.dev
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        for Es in (unsorted, np.linspace(eig.min(), eig.max(), 400), unsorted[:1]):
            for el in ("attached", "energy"):
                counts = {}
                for correction in (False, True):
                    dev.ctx.prof_reset()
                    a = rule.ltm(Es, states=True, elements=el, correction=correction)
                    counts[correction] = dev.ctx.prof_read(L.K_LTM)[1]
                    b = rule.ltm(Es, states=True, elements=el, correction=correction)
                    assert np.array_equal(a, b), (len(Es), el, correction)
                print(f"launches nE={len(Es)} {el}: plain {counts[False]}, corrected {counts[True]}")
                assert counts[True] == counts[False] >= 1
    finally:
        dev.ctx.prof_enable(False)
        rule.ltm_elements(None)


# ---------------------------------------------------------------- 7. refusals
def test_corrected_ltm_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s = cosine_series(abz, **MODEL_B)
    dev = s.device()
    Es = np.array([-0.5, 1.5])
    out = np.full(2 * 2, -99.0)
    pE, pout = Es.ctypes.data_as(L.c_f64p), out.ctypes.data_as(L.c_f64p)

    def untouched(rc, code):
        assert rc == code, (rc, code)
        assert len(lib.abz_last_error()) > 0
        assert np.all(out == -99.0)  # nothing was launched or written

    full = abz.DeviceRule(dev, 8, None, L.WANT_EIG)
    h = full._h
    untouched(lib.abz_rule_ltm_weighted(h, L.LTM_A_ELEMENTS, pE, 2, L.LTM_STATES_CORRECTED, pout), L.ERR_ARG)  # nothing attached
    assert full.ltm_elements_export() is None
    A = np.random.default_rng(3).standard_normal((2, full.nk, 1))
    full.ltm_elements(A)
    untouched(lib.abz_rule_ltm_weighted(h, L.LTM_A_ELEMENTS, pE, 2, 3, pout), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_weighted(h, L.LTM_A_ENERGY, pE, 2, 3, pout), L.ERR_ARG)
    untouched(lib.abz_rule_ltm_weighted(h, L.LTM_A_ELEMENTS, pE, 2, -1, pout), L.ERR_ARG)
    untouched(lib.abz_rule_ltm(h, pE, 2, L.LTM_STATES_CORRECTED, pout), L.ERR_ARG)  # the plain count has no correction
    assert np.array_equal(full.ltm_elements_export(), A)
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, 8, cub.syms, L.WANT_EIG)
    untouched(lib.abz_rule_ltm_weighted(sym._h, L.LTM_A_ENERGY, pE, 2, L.LTM_STATES_CORRECTED, pout), L.ERR_UNSUPPORTED)
    assert b"not a whole periodic grid" in lib.abz_last_error()
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, 8, 2, 6, L.WANT_EIG, C.byref(slab)))
    untouched(lib.abz_rule_ltm_weighted(slab, L.LTM_A_ENERGY, pE, 2, L.LTM_STATES_CORRECTED, pout), L.ERR_UNSUPPORTED)
    assert lib.abz_rule_destroy(slab) == 0
    # the attached elements are still in place, and a valid call works
    assert np.array_equal(full.ltm_elements_export(), A)
    assert lib.abz_rule_ltm_weighted(h, L.LTM_A_ELEMENTS, pE, 2, L.LTM_STATES_CORRECTED, pout) == 0
    eig = ln.rule_eigenvalues(full)
    ref = wn.wltm(eig, on_grid(full, A), Es)[1] + bn.correction(eig, on_grid(full, A), Es)
    check(out.reshape(2, 2), ref, "after the refusals")
    # the Python mirror keeps the refusal of a k-sharded rule
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        r = dev.rule(8, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm(Es, states=True, elements="energy", correction=True)
    finally:
        dev.kshard, dev.allreduce = None, None
    full.ltm_elements(None)

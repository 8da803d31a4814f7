"""Tetrahedron trace of the Green's function on the device (abz_rule_ltm_green, ltm_green_kernel<D, GreenTrace> in
kernels_ltm_green.hip) against the numpy restatement of tests/gltm_numpy.py and the reference's exact DOS formula.

Parity bound: the restatement is fed the rule's own exported eigenvalues, so only summation order, FMA contraction and the
device's log / atan2 remain; the bound is the LTM scans', |u - ref| <= 1e-9 max(1, max|ref|) (test_gpu_ltm.py), applied to the
real and the imaginary part.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import abz_oracle as orc
import gltm_numpy as gn
import ltm_numpy as ln
from test_ltm_green_cpu import FIVE
from test_oracle_pins import dos_integer_3d_exact

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 512  # values of z per launch (LTM_GREEN_CHUNK)


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def product_series(abz, so):
    return abz.FourierSeries(so.c, period=1.0, first=so.first, ndim=so.d)


def close(u, ref):
    """(deviation, bound) of the parity check, on the real and imaginary parts."""
    u, ref = np.asarray(u), np.asarray(ref)
    dev = max(np.abs(u.real - ref.real).max(), np.abs(u.imag - ref.imag).max())
    return dev, 1e-9 * max(1.0, np.abs(ref.real).max(), np.abs(ref.imag).max())


# ---------------------------------------------------------------- 5. parity with the restatement
CASES = {
    "int1_7": ("int1", 7), "int1_40": ("int1", 40), "int2_7": ("int2", 7), "graphene_12": ("graphene", 12),
    "int3_5": ("int3", 5),  # 125 cells: one ragged pass
    "int3_9": ("int3", 9),  # 729 cells: three passes
    "svo_8": ("svo", 8), "syn6_5": ("syn6", 5), "syn33_5": ("syn33", 5),
}


def make_series(abz, kind):
    if kind.startswith("int"):
        return product_series(abz, orc.tb_integer(int(kind[3:])))
    if kind == "graphene":
        return product_series(abz, orc.tb_graphene())
    if kind == "svo":
        return abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    return product_series(abz, orc.synthetic_wannier(int(kind[3:]), rmax=2, seed=7))


def z_lists(eig):
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    gamma = eig[(0,) * (eig.ndim - 1)]  # eigenvalues of the Gamma point (node 0)
    edges = np.concatenate([gamma, [lo, hi, hi + 1.0]])
    return {
        "one": np.array([lo + 0.37 * w + 1e-3j]),
        # unsorted, one duplicate, one value below the real axis
        "seven": np.array([lo + 0.7 * w + 1e-2j, lo + 0.1 * w + 0.5j, lo + 0.5 * w + 1e-4j, lo + 0.3 * w - 1e-2j, lo + 0.5 * w + 1e-4j,
                           hi + 0.3 * w + 1e-6j, lo - 0.1 * w + 2.0j]),
        "line300": np.linspace(lo - 0.05 * w, hi + 0.05 * w, 300) + 1e-2j,
        "two_chunks": np.linspace(lo - 0.1 * w, hi + 0.1 * w, CHUNK + 1) + 3e-2j,
        "edges": np.concatenate([edges + 1e-8j, edges + 0.3j]),
    }


@pytest.mark.parametrize("name", list(CASES))
def test_ltm_green_matches_restatement(abz, name):
    kind, npt = CASES[name]
    rule = make_series(abz, kind).device().rule(npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    e = ln.kuhn_simplices(eig)
    worst = 0.0
    for label, zs in z_lists(eig).items():
        u = rule.ltm_green(zs)
        ref = gn.green_trace(eig, zs, simplices=e)
        assert u.shape == ref.shape and u.dtype == np.complex128 and np.all(np.isfinite(u.view(np.float64))), (name, label)
        dev, bound = close(u, ref)
        print(f"ltm_green parity {name} {label} nz={len(zs)}: max dev {dev:.3e} (bound {bound:.1e})")
        assert dev <= bound, (name, label, dev, bound)
        worst = max(worst, dev / bound)
    print(f"ltm_green parity {name}: worst deviation / bound = {worst:.3e}")


# ---------------------------------------------------------------- 6. conjugation and repeatability, to the bit
def test_ltm_green_conjugate_and_repeatable(abz):
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    rule = s.device().rule(8, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    rng = np.random.default_rng(3)
    zs = eig.min() + (eig.max() - eig.min()) * rng.random(67) + 1j * 10.0 ** rng.uniform(-8, 0, 67)
    a, b = rule.ltm_green(zs), rule.ltm_green(zs)
    assert np.array_equal(a.view(np.float64), b.view(np.float64))
    c = rule.ltm_green(np.conj(zs))
    assert np.array_equal(np.conj(a).view(np.float64), c.view(np.float64))
    mixed = np.where(np.arange(67) % 2 == 0, zs, np.conj(zs))
    m = rule.ltm_green(mixed)
    assert np.array_equal(np.where(np.arange(67) % 2 == 0, a, np.conj(a)).view(np.float64), m.view(np.float64))
    assert np.all(a.imag < 0.0) and np.all(c.imag > 0.0)


# ---------------------------------------------------------------- 7. unfolded rule
def test_ltm_green_on_an_unfolded_rule(abz):
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    full = dev.rule(8, None, abz._lib.WANT_EIG)
    unf = dev.rule(8, cub.syms, abz._lib.WANT_EIG).unfold()
    zs = np.linspace(-6.5, 6.5, 41) + 1e-3j
    a, b = full.ltm_green(zs), unf.ltm_green(zs)
    dv, bound = close(b, a)
    print(f"ltm_green unfolded vs full grid: max dev {dv:.3e} (bound {bound:.1e})")
    assert dv <= bound


# ---------------------------------------------------------------- 8. end to end
def test_ltm_eta_end_to_end(abz):
    s = product_series(abz, orc.tb_integer(3))
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    Es = np.array(FIVE)
    eta = 1e-3
    cache = abz.dos.init(abz.DOSProblem(s, Es, bz), abz.LTM(npt=48, eta=eta))
    u = abz.dos.solve_(cache).u
    exact = np.array([dos_integer_3d_exact(E) for E in FIVE])
    err = np.abs(u - exact).max()
    print(f"LTM(npt=48, eta=1e-3) vs exact DOS: max err {err:.3e}")
    assert u.shape == (5,) and err <= 1e-2
    t = abz.dos.green_trace(cache, Es + 1j * eta)
    assert np.array_equal(-t.imag / np.pi, u)
    one = abz.dos.solve(abz.DOSProblem(s, float(Es[2]), bz), abz.LTM(npt=48, eta=eta)).u
    assert isinstance(one, float) and one == u[2]
    sym = abz.dos.solve(abz.DOSProblem(s, Es, abz.load_bz(abz.CubicSymIBZ(), np.eye(3))), abz.LTM(npt=48, eta=eta, symmetric=True)).u
    assert np.abs(sym - u).max() <= 1e-9 * max(1.0, np.abs(u).max())
    g = abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=48)).u  # the plain scan next to it: the eta -> 0 limit
    assert np.abs(u - g).max() <= 1e-3


def test_green_trace_follows_the_series(abz):
    """dos.green_trace on a cache refreshes like the elements caches: mutate in place and set isfresh, then assign a new H."""
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    bz = abz.load_bz(abz.FBZ(), [[2 * np.pi]])
    zs = np.array([0.3 + 1e-2j, -0.7 + 1e-4j])
    cache = abz.dos.init(abz.DOSProblem(h, 0.3, bz), abz.LTM())
    k = np.arange(50) / 50.0

    def expect(scale):
        eig = ln.rule_eigenvalues(cache.cacheval)
        assert np.abs(eig - (scale * np.cos(2 * np.pi * k))[:, None]).max() <= 1e-12 * scale
        return gn.green_trace(eig, zs)

    t1 = abz.dos.green_trace(cache, zs)
    r1 = expect(1.0)
    assert close(t1, r1)[0] <= close(t1, r1)[1]
    h.c *= 2
    cache.isfresh = True
    t2 = abz.dos.green_trace(cache, zs)
    r2 = expect(2.0)
    assert close(t2, r2)[0] <= close(t2, r2)[1] and np.abs(r2 - r1).max() > 1e-3
    cache.H = abz.FourierSeries(2 * h.c, period=1.0, offset=-2)
    assert cache.isfresh
    t3 = abz.dos.green_trace(cache, zs)
    r3 = expect(4.0)
    assert close(t3, r3)[0] <= close(t3, r3)[1] and np.abs(r3 - r2).max() > 1e-3
    assert not cache.isfresh
    # a problem instead of a cache
    t4 = abz.dos.green_trace(abz.DOSProblem(cache.H, 0.0, bz), zs)
    assert np.array_equal(t4.view(np.float64), t3.view(np.float64))


# ---------------------------------------------------------------- 9. refusals
def test_ltm_green_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    zs = np.array([0.5 + 1e-2j, 1.5 + 1e-3j])
    out = np.full(4, -99.0)
    pz, pout = zs.view(np.float64).ctypes.data_as(L.c_f64p), out.ctypes.data_as(L.c_f64p)

    def refused(h, code, nz=2, z=pz, o=pout):
        assert lib.abz_rule_ltm_green(h, z, nz, o) == code
        assert len(lib.abz_last_error()) > 0
        assert np.all(out == -99.0)  # nothing was launched or written

    full = abz.DeviceRule(dev, 8, None, L.WANT_EIG)
    for bad in (0.5 + 0.0j, complex(float("nan"), 1e-2), complex(0.5, float("inf")), complex(0.5, float("nan"))):
        zb = np.array([0.5 + 1e-2j, bad])
        refused(full._h, L.ERR_ARG, z=zb.view(np.float64).ctypes.data_as(L.c_f64p))
    refused(full._h, L.ERR_ARG, nz=0)
    refused(full._h, L.ERR_ARG, z=None)
    refused(full._h, L.ERR_ARG, o=None)
    honly = abz.DeviceRule(dev, 8, None, L.WANT_H)
    refused(honly._h, L.ERR_ARG)
    # a valid call afterwards still works
    assert lib.abz_rule_ltm_green(full._h, pz, 2, pout) == 0
    ref = gn.green_trace(ln.rule_eigenvalues(full), zs)
    dv, bound = close(out.view(np.complex128), ref)
    assert dv <= bound
    out[:] = -99.0
    # a slab, without and with its halo plane
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, 8, 2, 6, L.WANT_EIG, C.byref(slab)))
    refused(slab, L.ERR_UNSUPPORTED)
    L.check(lib.abz_rule_ltm_halo(slab))
    refused(slab, L.ERR_UNSUPPORTED)
    Es, g = np.array([0.5, 1.5]), np.zeros(2)
    assert lib.abz_rule_ltm(slab, Es.ctypes.data_as(L.c_f64p), 2, L.LTM_DOS, g.ctypes.data_as(L.c_f64p)) == 0 and np.all(g > 0.0)
    # a symmetric rule and a list of irreducible nodes; both still unfold afterwards, and the unfolded rule is taken
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, 8, cub.syms, L.WANT_EIG)
    refused(sym._h, L.ERR_UNSUPPORTED)
    dv, bound = close(sym.unfold().ltm_green(zs), ref)
    assert dv <= bound
    idx, w = abz.symptr_rule(8, 3, cub.syms)
    irr = C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, 8, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(irr)))
    refused(irr, L.ERR_UNSUPPORTED)
    S = np.ascontiguousarray(np.rint(np.asarray(cub.syms)).astype(np.int32).reshape(-1, 3, 3))
    unf = C.c_void_p()
    L.check(lib.abz_rule_ltm_unfold(irr, S.ctypes.data_as(L.c_i32p), len(S), C.byref(unf)))
    assert lib.abz_rule_ltm_green(unf, pz, 2, pout) == 0
    dv, bound = close(out.view(np.complex128), ref)
    assert dv <= bound
    assert lib.abz_rule_destroy(unf) == 0 and lib.abz_rule_destroy(irr) == 0 and lib.abz_rule_destroy(slab) == 0
    # the Python mirror on a k-sharded device, without and with the halo plane; nothing is built for dos.green_trace
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        rule = dev.rule(8, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError):
            rule.ltm_green(zs)
        rule.ltm_halo()
        with pytest.raises(NotImplementedError, match="ltm_green"):
            rule.ltm_green(zs)
        bz = abz.load_bz(abz.FBZ(), np.eye(3))
        with pytest.raises(NotImplementedError):
            abz.dos.green_trace(abz.DOSProblem(s, 0.0, bz), zs)
        with pytest.raises(NotImplementedError):
            abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=8, eta=0.1))
    finally:
        dev.kshard, dev.allreduce = None, None
    with pytest.raises(ValueError, match="real"):
        full.ltm_green([0.5])  # real z through the mirror


# ---------------------------------------------------------------- 10. profiling slot
def test_ltm_green_profiling_slot(abz):
    """The launches are counted under K_LTM: one scope per chunk of z."""
    L = abz._lib
    s = product_series(abz, orc.tb_integer(2))
    dev = s.device()
    rule = dev.rule(16, None, L.WANT_EIG)
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        dev.ctx.prof_reset()
        rule.ltm_green(np.linspace(-3, 3, 10) + 1e-2j)
        ms, launches = dev.ctx.prof_read(L.K_LTM)
        assert launches == 1 and ms > 0.0
        rule.ltm_green(np.linspace(-3, 3, CHUNK + 1) + 1e-2j)
        assert dev.ctx.prof_read(L.K_LTM)[1] == launches + 2
        assert dev.ctx.prof_read(L.K_GGR)[1] == 0
    finally:
        dev.ctx.prof_enable(False)

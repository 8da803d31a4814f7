"""Tetrahedron Green's function with matrix elements on the device (abz_rule_ltm_green_weighted, ltm_green_kernel<D, GreenElems<NC>> in
kernels_ltm_green.hip) against the numpy restatement of tests/gwltm_numpy.py, its own identities and the trace abz_rule_ltm_green.

Parity bound: the restatement is fed the rule's own exported eigenvalues and elements, so only summation order, FMA contraction
and the device's log / atan2 remain; the bound is the LTM scans', |u - ref| <= 1e-9 max(1, max|ref|) (test_gpu_ltm.py), applied to
the real and the imaginary part.

The restatement costs 6 ... 250 ms per value of z.  The list that crosses a z chunk is therefore compared with it at every
STRIDE-th value only, and in full -- to the bit -- with the same values computed by the device in two shorter calls, neither of
which crosses a chunk: a value of z is summed in the same order whatever list it came in, so a chunk boundary that moved, lost or
mixed a value shows there.  For the same reason the 33-band case thins the `edges` list to every fourth eigenvalue of the Gamma
point: what that case adds is the launch geometry of many bands, not another simplex formula.
"""
import ctypes as C
import os

import numpy as np
import pytest

import abz_oracle as orc
import gwltm_numpy as gw
import ltm_numpy as ln
from test_gpu_ltm_green import close, make_series, product_series
from test_gpu_ltm_weighted import on_grid

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK4 = 154  # values of z per launch of a group of 4 components, the smallest chunk (green_w_chunk(4)); 291 for 2, 512 for 1


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def check(u, ref, what):
    u, ref = np.ascontiguousarray(u), np.ascontiguousarray(ref)
    assert u.shape == ref.shape and u.dtype == np.complex128 and np.all(np.isfinite(u.view(np.float64))), (what, u.shape, ref.shape)
    dev, bound = close(u, ref)
    print(f"ltm_green weighted {what}: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)
    return dev / bound


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def z_lists(eig, thin=1):
    """The lists of the trace's test: one, seven (unsorted, a duplicate, one value below the real axis), the band edges and the
    Gamma point's eigenvalues at 1e-8, and a list one longer than the smallest z chunk."""
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    gamma = eig[(0,) * (eig.ndim - 1)]  # eigenvalues of the Gamma point (node 0)
    edges = np.concatenate([gamma[::thin], [lo, hi, hi + 1.0]])
    return {
        "one": np.array([lo + 0.37 * w + 1e-3j]),
        "seven": np.array([lo + 0.7 * w + 1e-2j, lo + 0.1 * w + 0.5j, lo + 0.5 * w + 1e-4j, lo + 0.3 * w - 1e-2j, lo + 0.5 * w + 1e-4j,
                           hi + 0.3 * w + 1e-6j, lo - 0.1 * w + 2.0j]),
        "edges": edges + 1e-8j,
        "chunk": np.linspace(lo - 0.1 * w, hi + 0.1 * w, CHUNK4 + 1) + 3e-2j,
    }


# ---------------------------------------------------------------- 1. parity with the restatement
# name: (series, npt, elements, stride of the chunk list against the restatement, thinning of the Gamma eigenvalues)
CASES = {
    "int1_7": ("int1", 7, "energy", 1, 1),
    "int2_7": ("int2", 7, "energy", 1, 1),
    "graphene_12": ("graphene", 12, ("orbitals", None), 4, 1),   # 2 device orbitals: a group of 2
    "int3_5": ("int3", 5, ("random", 7), 8, 1),                  # 125 cells: one ragged pass; groups 4 + 2 + 1
    "int3_9": ("int3", 9, ("random", 4), 16, 1),                 # 729 cells: three passes; a group of 4
    "svo_8": ("svo", 8, ("orbitals", None), 16, 1),              # 3 device orbitals: groups 2 + 1
    "syn33_5": ("syn33", 5, "energy", 31, 4),                    # the 33-band path
}


def attach(rule, elements, seed=11):
    """Attach what the case asks for; -> (the `elements` argument of ltm_green, the elements on the grid for the restatement)."""
    eig = ln.rule_eigenvalues(rule)
    if elements == "energy":
        return "energy", eig[None]
    kind, arg = elements
    if kind == "orbitals":
        rule.ltm_orbitals(arg)
    else:
        rule.ltm_elements(np.random.default_rng(seed).uniform(-1.0, 1.0, (arg, rule.nk, rule.dev.s.n)))
    return "attached", on_grid(rule, rule.ltm_elements_export())


@pytest.mark.parametrize("name", list(CASES))
def test_ltm_green_weighted_matches_restatement(abz, name):
    kind, npt, elements, stride, thin = CASES[name]
    rule = make_series(abz, kind).device().rule(npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    el, A = attach(rule, elements)
    ncomp = A.shape[0]
    worst = 0.0
    for label, zs in z_lists(eig, thin).items():
        u = rule.ltm_green(zs, elements=el)
        assert u.shape == (len(zs), ncomp), (name, label, u.shape)
        sub = slice(None, None, stride) if label == "chunk" else slice(None)
        worst = max(worst, check(u[sub], gw.green_weighted(eig, A, zs[sub]), f"parity {name} {label} nz={len(zs)}"))
        if label == "chunk":  # the whole list, to the bit, against two calls that do not cross a chunk
            h = len(zs) // 2
            two = np.concatenate([rule.ltm_green(zs[:h], elements=el), rule.ltm_green(zs[h:], elements=el)])
            assert np.array_equal(bits(u), bits(two)), (name, label)
    print(f"ltm_green weighted parity {name}: worst deviation / bound = {worst:.3e}")


# ---------------------------------------------------------------- 2. identities on the device
def test_ltm_green_weighted_identities(abz):
    """A = e gives z tr G(z) - n (|z| within twice the bandwidth), A = 1 gives tr G(z), and the orbital weights of all orbitals
    sum to tr G(z)."""
    rule = product_series(abz, orc.tb_integer(3)).device().rule(8, None, abz._lib.WANT_EIG)
    rng = np.random.default_rng(7)
    flip = np.where(np.arange(40) % 5 == 0, -1.0, 1.0)
    zs = rng.uniform(-14.0, 14.0, 40) + 1j * flip * 10.0 ** rng.uniform(-4, 0, 40)  # the band is [-6, 6]
    assert np.abs(zs).max() <= 24.0
    t = rule.ltm_green(zs)
    ge = rule.ltm_green(zs, elements="energy")
    assert ge.shape == (40, 1)
    check(ge[:, 0], zs * t - 1.0, "A = e against z tr G - n")
    check(rule.ltm_green(zs, elements=np.ones((1, rule.nk, 1)))[:, 0], t, "A = 1 against the trace")
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    rule = s.device().rule(8, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    zs = eig.min() + (eig.max() - eig.min()) * rng.uniform(-0.2, 1.2, 40) + 1j * flip * 10.0 ** rng.uniform(-4, 0, 40)
    rule.ltm_orbitals()
    go = rule.ltm_green(zs, elements="attached")
    assert go.shape == (40, 3)
    check(go.sum(axis=1), rule.ltm_green(zs), "sum of the three orbital weights against the trace")


def test_ltm_green_weighted_routes_components(abz):
    """Two uncoupled copies of tb_integer(2) at -Delta and +Delta, Delta above the bandwidth (8): the bands never cross,
    orbital 0 is the lower band everywhere.  G_00(z) is the one-band trace at z + Delta, G_11(z) that at z - Delta, not swapped."""
    D = 16.0
    one = orc.tb_integer(2)
    c = np.zeros((3, 3, 2, 2))
    c[:, :, 0, 0] = one.c[:, :, 0, 0].real
    c[:, :, 1, 1] = one.c[:, :, 0, 0].real
    c[1, 1, 0, 0], c[1, 1, 1, 1] = -D, D
    two = abz.FourierSeries(c, period=1.0, first=one.first, ndim=2).device().rule(9, None, abz._lib.WANT_EIG)
    ref = product_series(abz, one).device().rule(9, None, abz._lib.WANT_EIG)
    two.ltm_orbitals()
    x = np.array([-3.5, -0.25, 0.0, 1.75, 4.5])
    zs = np.concatenate([x - D, x + D]) + np.tile([1e-2j, 1e-4j, -1e-3j, 0.5j, 1e-6j], 2)
    G = two.ltm_green(zs, elements="attached")
    assert G.shape == (10, 2)
    r0, r1 = ref.ltm_green(zs + D), ref.ltm_green(zs - D)
    check(G[:, 0], r0, "G_00(z) against the one-band trace at z + Delta")
    check(G[:, 1], r1, "G_11(z) against the one-band trace at z - Delta")
    assert np.abs(G[:, 0] - r1).max() > 1e-2 and np.abs(G[:, 1] - r0).max() > 1e-2  # (a swap would pass the sum)
    # the reversed selection reverses the columns, to the bit
    two.ltm_orbitals([1, 0])
    assert np.array_equal(bits(two.ltm_green(zs, elements="attached")), bits(G[:, ::-1]))


# ---------------------------------------------------------------- 3. conjugation and repeatability, to the bit
def test_ltm_green_weighted_conjugate_and_repeatable(abz):
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    rule = s.device().rule(8, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    rng = np.random.default_rng(3)
    zs = eig.min() + (eig.max() - eig.min()) * rng.random(67) + 1j * 10.0 ** rng.uniform(-8, 0, 67)
    rule.ltm_elements(rng.uniform(-1.0, 1.0, (7, rule.nk, 3)))
    even = (np.arange(67) % 2 == 0)
    for el in ("energy", "attached"):
        a, b = rule.ltm_green(zs, elements=el), rule.ltm_green(zs, elements=el)
        assert np.array_equal(bits(a), bits(b))
        c = rule.ltm_green(np.conj(zs), elements=el)
        assert np.array_equal(bits(np.conj(a)), bits(c))
        m = rule.ltm_green(np.where(even, zs, np.conj(zs)), elements=el)
        assert np.array_equal(bits(np.where(even[:, None], a, np.conj(a))), bits(m))
    # None stays the trace, shape [nz]
    assert rule.ltm_green(zs).shape == (67,)


# ---------------------------------------------------------------- 4. unfolded rule
def test_ltm_green_weighted_on_an_unfolded_rule(abz):
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    full = dev.rule(8, None, abz._lib.WANT_EIG)
    unf = dev.rule(8, cub.syms, abz._lib.WANT_EIG).unfold()
    zs = np.linspace(-6.5, 6.5, 41) + 1e-3j
    check(unf.ltm_green(zs, elements="energy"), full.ltm_green(zs, elements="energy"), "unfolded against full grid, energy")
    # elements of a callable, attached at the full-grid nodes of either rule: not invariant under the cube's symmetries
    elements = lambda x, eig: np.stack([np.cos(2 * np.pi * x[:, :1]) ** 2 + 0 * eig, np.sin(2 * np.pi * (x[:, 1:2] + 2 * x[:, 2:3])) + 0.1 * eig])
    out = []
    for rule in (full, unf):
        ex = rule.export(x=True, w=False, eig=True)
        out.append(rule.ltm_green(zs, elements=np.ascontiguousarray(elements(ex["x"], ex["eig"]))))
    assert out[0].shape == (41, 2)
    check(out[1], out[0], "unfolded against full grid, elements of a callable")


# ---------------------------------------------------------------- 5. end to end
def test_ltm_eta_elements_end_to_end(abz):
    h = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    bz = abz.load_bz(abz.FBZ(), 3.85856 * np.eye(3))
    eta = 1e-2
    alg = abz.LTM(npt=8, eta=eta, elements="orbitals", eigenvectors="device")
    eig0 = ln.rule_eigenvalues(h.device().rule(8, None, abz._lib.WANT_EIG))
    Es = np.linspace(eig0.min() - 0.1, eig0.max() + 0.1, 9)
    cache = abz.dos.init(abz.DOSProblem(h, Es, bz), alg)

    def expect():
        rule = cache.cacheval
        eig = ln.rule_eigenvalues(rule)
        return eig, -gw.green_weighted(eig, on_grid(rule, rule.ltm_elements_export()), Es + 1j * eta).imag / np.pi

    u = abz.dos.solve_(cache).u
    assert u.shape == (9, 3)
    G = abz.dos.green_weighted(cache, Es + 1j * eta)
    assert G.shape == (9, 3) and np.array_equal(-G.imag / np.pi, u)
    eig1, r1 = expect()
    dv, bound = close(u + 0j, r1 + 0j)
    print(f"LTM(eta, orbitals) end to end: max dev {dv:.3e} (bound {bound:.1e})")
    assert dv <= bound
    # the trace next to it
    tr = abz.dos.solve(abz.DOSProblem(h, Es, bz), abz.LTM(npt=8, eta=eta)).u
    assert np.abs(u.sum(axis=1) - tr).max() <= 1e-9 * max(1.0, tr.max())
    # a scalar domain
    one = abz.dos.solve(abz.DOSProblem(h, float(Es[4]), bz), alg).u
    assert one.shape == (3,) and np.array_equal(one, u[4])
    # "energy" and a selection of orbitals
    ue = abz.dos.solve(abz.DOSProblem(h, Es, bz), abz.LTM(npt=8, eta=eta, elements="energy")).u
    assert ue.shape == (9, 1)
    sel = abz.dos.solve(abz.DOSProblem(h, Es, bz), abz.LTM(npt=8, eta=eta, elements="orbitals", eigenvectors="device", orbitals=[2])).u
    assert sel.shape == (9, 1)
    dv, bound = close(sel[:, 0] + 0j, u[:, 2] + 0j)
    assert dv <= bound
    # mutate in place and set isfresh: the elements are recomputed and the result follows
    h.c[...] = h.c * 0.5
    cache.isfresh = True
    u2 = abz.dos.solve_(cache).u
    eig2, r2 = expect()
    assert not cache.isfresh and np.abs(eig2 - 0.5 * eig1).max() <= 1e-9 * np.abs(eig1).max()
    dv, bound = close(u2 + 0j, r2 + 0j)
    assert dv <= bound and np.abs(u2 - u).max() > 1e-3
    cache.isfresh = True
    G2 = abz.dos.green_weighted(cache, Es + 1j * eta)
    assert not cache.isfresh and np.array_equal(-G2.imag / np.pi, u2)
    # a cache without elements, and a problem instead of a cache ("energy")
    with pytest.raises(ValueError):
        abz.dos.green_weighted(abz.dos.init(abz.DOSProblem(h, Es, bz), abz.LTM(npt=8)), Es + 1j * eta)
    Gp = abz.dos.green_weighted(abz.DOSProblem(h, 0.0, bz), Es[:2] + 1j * eta)
    assert Gp.shape == (2, 1)


# ---------------------------------------------------------------- 6. refusals
def test_ltm_green_weighted_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    zs = np.array([0.5 + 1e-2j, 1.5 + 1e-3j])
    out = np.full(8, -99.0)
    pz, pout = zs.view(np.float64).ctypes.data_as(L.c_f64p), out.ctypes.data_as(L.c_f64p)

    def refused(h, code, source=L.LTM_A_ENERGY, nz=2, z=pz, o=pout):
        assert lib.abz_rule_ltm_green_weighted(h, source, z, nz, o) == code
        assert len(lib.abz_last_error()) > 0
        assert np.all(out == -99.0)  # nothing was launched or written

    full = abz.DeviceRule(dev, 8, None, L.WANT_EIG)
    for bad in (0.5 + 0.0j, complex(float("nan"), 1e-2), complex(0.5, float("inf")), complex(0.5, float("nan"))):
        zb = np.array([0.5 + 1e-2j, bad])
        refused(full._h, L.ERR_ARG, z=zb.view(np.float64).ctypes.data_as(L.c_f64p))
    refused(full._h, L.ERR_ARG, nz=0)
    refused(full._h, L.ERR_ARG, z=None)
    refused(full._h, L.ERR_ARG, o=None)
    refused(full._h, L.ERR_ARG, source=2)
    refused(full._h, L.ERR_ARG, source=-1)
    refused(full._h, L.ERR_ARG, source=L.LTM_A_ELEMENTS)  # nothing attached
    honly = abz.DeviceRule(dev, 8, None, L.WANT_H)
    refused(honly._h, L.ERR_ARG)
    # a valid call afterwards still works, with the energy and with attached elements
    eig = ln.rule_eigenvalues(full)
    assert lib.abz_rule_ltm_green_weighted(full._h, L.LTM_A_ENERGY, pz, 2, pout) == 0
    ref = gw.green_weighted(eig, eig, zs)
    check(out[:4].view(np.complex128).reshape(2, 1), ref, "a valid call after the refusals")
    assert np.all(out[4:] == -99.0)
    A = np.random.default_rng(2).uniform(-1.0, 1.0, (2, full.nk, 1))
    full.ltm_elements(A)
    assert lib.abz_rule_ltm_green_weighted(full._h, L.LTM_A_ELEMENTS, pz, 2, pout) == 0
    refA = gw.green_weighted(eig, on_grid(full, A), zs)
    check(out.view(np.complex128).reshape(2, 2), refA, "attached elements through the C call")
    out[:] = -99.0
    # a slab, without and with its halo plane
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, 8, 2, 6, L.WANT_EIG, C.byref(slab)))
    refused(slab, L.ERR_UNSUPPORTED)
    L.check(lib.abz_rule_ltm_halo(slab))
    refused(slab, L.ERR_UNSUPPORTED)
    refused(slab, L.ERR_UNSUPPORTED, source=L.LTM_A_ELEMENTS)
    # a symmetric rule and a list of irreducible nodes; the unfolded rule is taken
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, 8, cub.syms, L.WANT_EIG)
    refused(sym._h, L.ERR_UNSUPPORTED)
    check(sym.unfold().ltm_green(zs, elements="energy"), ref, "the unfolded rule")
    idx, w = abz.symptr_rule(8, 3, cub.syms)
    irr = C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, 8, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(irr)))
    refused(irr, L.ERR_UNSUPPORTED)
    assert lib.abz_rule_destroy(irr) == 0 and lib.abz_rule_destroy(slab) == 0
    # the Python mirror
    with pytest.raises(ValueError, match="real"):
        full.ltm_green([0.5], elements="energy")
    with pytest.raises(ValueError):
        full.ltm_green(zs, elements="orbitals")
    full.ltm_elements(None)
    with pytest.raises(ValueError, match="attached"):
        full.ltm_green(zs, elements="attached")
    # ... on a k-sharded device, without and with the halo plane; nothing is built for dos.green_weighted
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        rule = dev.rule(8, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError):
            rule.ltm_green(zs, elements="energy")
        rule.ltm_halo()
        with pytest.raises(NotImplementedError, match="ltm_green"):
            rule.ltm_green(zs, elements="energy")
        bz = abz.load_bz(abz.FBZ(), np.eye(3))
        with pytest.raises(NotImplementedError):
            abz.dos.green_weighted(abz.DOSProblem(s, 0.0, bz), zs)
        with pytest.raises(NotImplementedError):
            abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=8, eta=0.1, elements="energy"))
    finally:
        dev.kshard, dev.allreduce = None, None


# ---------------------------------------------------------------- 7. profiling slot
def test_ltm_green_weighted_profiling_slot(abz):
    """The launches are counted under K_LTM: one scope per (component group, chunk of z)."""
    L = abz._lib
    s = product_series(abz, orc.tb_integer(2))
    dev = s.device()
    rule = dev.rule(16, None, L.WANT_EIG)
    rule.ltm_elements(np.random.default_rng(4).uniform(-1.0, 1.0, (7, rule.nk, 1)))
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        dev.ctx.prof_reset()
        rule.ltm_green(np.linspace(-3, 3, 10) + 1e-2j, elements="energy")
        ms, launches = dev.ctx.prof_read(L.K_LTM)
        assert launches == 1 and ms > 0.0
        rule.ltm_green(np.linspace(-3, 3, 10) + 1e-2j, elements="attached")  # groups 4 + 2 + 1
        assert dev.ctx.prof_read(L.K_LTM)[1] == launches + 3
        launches += 3
        rule.ltm_green(np.linspace(-3, 3, CHUNK4 + 1) + 1e-2j, elements="attached")  # 2 chunks of the 4, 1 of the 2 and the 1
        assert dev.ctx.prof_read(L.K_LTM)[1] == launches + 4
        assert dev.ctx.prof_read(L.K_GGR)[1] == 0
    finally:
        dev.ctx.prof_enable(False)

"""Orbital weights |U_ab(k)|^2 computed on the device as matrix elements of the tetrahedron method
(abz_rule_ltm_orbitals, kernels_ltm_orb.hip), their way back to the host (abz_rule_ltm_elements_export), and the
`eigenvectors="device"` route of LTM(elements="orbitals"), against LAPACK (tests/orbw_numpy.py), the geometric restatement of
the weighted scan (tests/wltm_numpy.py) and the host route.

Bounds.  Separated bands: the models' smallest gap between neighbouring bands on the grids used is 0.0158 (n = 12; 0.0209 at
n = 16) at a spectrum scale of about 5; first-order perturbation theory puts the eigenvector error at n eps ||H|| / gap, about
1e-12, and the bound on the weights is 1e-10.  Degenerate levels: any orthonormal basis of the eigenspace is an answer
(ref: src/dos_ggr.jl:31-44), so only sums over a level and the two normalisations are compared, to 1e-8, the project's bound
for eigenvector-derived sums (test_gpu_parity.py::test_ggr_rows_degenerate_bands).  Scans: the restatement is fed the
exported eigenvalues and the exported DEVICE weights, so the bound is the LTM parity bound 1e-9 max(1, max|ref|)."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import abz_oracle as orc
import ltm_numpy as ln
import orbw_numpy as ow
import wltm_numpy as wn
from test_gpu_ltm import GOLD, close, energy_lists, make_case, product_series
from test_gpu_ltm_weighted import check, on_grid
from test_gpu_parity import rand_series

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def device_weights(rule, orbitals=None):
    rule.ltm_orbitals(orbitals)
    W = rule.ltm_elements_export()
    n = rule.dev.s.n
    assert W.shape == ((n if orbitals is None else len(orbitals)), rule.nk, n) and np.all(np.isfinite(W))
    return W


def check_weights(abz, s, npt, what, orbitals=None):
    """Device weights of a rule with H and eigenvalues against LAPACK on the exported H.  Returns the largest deviation."""
    L = abz._lib
    rule = abz.DeviceRule(s.device(), npt, None, L.WANT_H | L.WANT_EIG)
    try:
        H = rule.export(x=False, w=False, H=True)["H"]
        ref = ow.weights(H)
        W = device_weights(rule, orbitals)
        full = orbitals is None
        dev = np.abs(W - (ref if full else ref[list(orbitals)])).max()
        colsum = np.abs((W if full else device_weights(rule)).sum(axis=0) - 1.0).max() if ref.shape[0] <= 16 else 0.0
        rowsum = np.abs(W.sum(axis=2) - 1.0).max()  # sum over the bands of every requested orbital
        print(f"orbital weights {what} npt={npt}: max dev {dev:.3e}, |sum_a - 1| {colsum:.3e}, |sum_b - 1| {rowsum:.3e}")
        assert dev <= 1e-10 and colsum <= 1e-10 and rowsum <= 1e-10, (what, npt, dev, colsum, rowsum)
        return dev
    finally:
        rule.close()


# ---------------------------------------------------------------- 1. weights against LAPACK, separated bands
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 12, 16])
def test_orbital_weights_match_lapack(abz, n):
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    for npt in (5, 12):
        check_weights(abz, s, npt, f"syn{n}")


@pytest.mark.parametrize("n", [17, 24])
def test_orbital_weights_match_lapack_17_to_32_bands(abz, n):
    """Above 16 bands a selection of at most 16 orbitals: sixteen of them, out of order, the last one included."""
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    orbitals = [n - 1, 0, 5, 3] + list(range(6, 17)) + [1]
    assert len(orbitals) == 16 and max(orbitals) == n - 1
    for npt in (5, 12):
        check_weights(abz, s, npt, f"syn{n}", orbitals)


@pytest.mark.parametrize("d,dims,npts", [(1, (5,), (9, 40)), (2, (3, 5), (7,))])
def test_orbital_weights_in_one_and_two_dimensions(abz, d, dims, npts):
    rng = np.random.default_rng(100 * d + 6)
    c, first = rand_series(rng, dims, 6, hermitian=True)
    s = abz.FourierSeries(c, period=1.0, first=first, ndim=d)
    for npt in npts:
        check_weights(abz, s, npt, f"{d}-D 6 bands")


def test_orbital_weight_of_a_scalar_series_is_one(abz):
    s = product_series(abz, orc.tb_integer(2))
    for want in (abz._lib.WANT_EIG, abz._lib.WANT_H | abz._lib.WANT_EIG):
        rule = abz.DeviceRule(s.device(), 9, None, want)
        W = device_weights(rule)
        assert W.shape == (1, 81, 1) and np.all(W == 1.0)
        rule.close()


# ---------------------------------------------------------------- 2. layouts
@pytest.mark.parametrize("n", [3, 6, 12, 17])
def test_orbital_weights_do_not_depend_on_the_h_layout(abz, n):
    """One lane kernel and the row kernels of 8, 16 and 32 lanes per node; above 16 bands the selection of sixteen orbitals of
    test_orbital_weights_match_lapack_17_to_32_bands.  The library has no compact layout above 16 bands and drops the bit
    (abzhip.h): at n = 17 the third rule is a second full-layout one, so the case checks the transient H against the resident
    one at 32 lanes per node, not the compact branch."""
    L = abz._lib
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    orbitals = None if n <= 16 else [n - 1, 0, 5, 3] + list(range(6, 17)) + [1]
    blocks = []
    for want in (L.WANT_EIG, L.WANT_H | L.WANT_EIG, L.WANT_H | L.WANT_EIG | L.WANT_H_COMPACT):
        rule = abz.DeviceRule(s.device(), 12, None, want)
        W = device_weights(rule, orbitals)
        assert np.array_equal(W, device_weights(rule, orbitals)), want  # two calls on one rule
        if want == L.WANT_EIG:
            asked = list(range(n)) if orbitals is None else orbitals
            sel = device_weights(rule, [asked[2], asked[0], asked[2]])
            assert np.array_equal(sel, W[[2, 0, 2]])
        blocks.append(W)
        rule.close()
    assert np.array_equal(blocks[0], blocks[1]) and np.array_equal(blocks[0], blocks[2])


# ---------------------------------------------------------------- 3. degenerate levels
@pytest.mark.parametrize("n3,mult", [(3, 2), (2, 4), (3, 3), (4, 4)])
def test_orbital_weights_of_degenerate_levels(abz, n3, mult):
    """H = Q (I_mult x h(k)) Q^H, every level `mult` times (test_ggr_rows_degenerate_bands): sums of the weights over each
    level against LAPACK's, both normalisations at every node."""
    L = abz._lib
    rng = np.random.default_rng(7 * n3 + mult)
    c3, first = rand_series(rng, (3, 3, 3), n3, hermitian=True)
    n = n3 * mult
    q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    c = np.einsum("ab,...bc,dc->...ad", q, np.kron(np.eye(mult), c3), q.conj())
    # the rotation leaves c(-R) = c(R)^dagger true to rounding only; the entry point asks for it exactly (the library's test of a
    # Hermitian series), so the two halves are averaged: the levels stay degenerate to rounding, which is the case under test
    c = 0.5 * (c + np.conj(np.swapaxes(c[::-1, ::-1, ::-1], -1, -2)))
    s = abz.FourierSeries(c, period=1.0, first=first)
    for npt in (5, 19):
        rule = abz.DeviceRule(s.device(), npt, None, L.WANT_H | L.WANT_EIG)
        ex = rule.export(x=False, w=False, H=True, eig=True)
        e = ex["eig"]
        W = device_weights(rule)
        rule.close()
        scale = np.abs(e).max()
        e3 = e.reshape(len(e), n3, mult)[:, :, 0]
        sep = np.min(np.diff(e3, axis=1), axis=1) > 1e-6 * scale
        assert sep.mean() > 0.9
        got = ow.cluster_sums(e[sep], W[:, sep], 1e-6 * scale)
        ref = ow.cluster_sums(e[sep], ow.weights(ex["H"][sep]), 1e-6 * scale)
        dev = np.abs(got - ref).max()
        colsum, rowsum = np.abs(W.sum(axis=0) - 1.0).max(), np.abs(W.sum(axis=2) - 1.0).max()
        print(f"degenerate levels {n3} x {mult} npt={npt}: level sums {dev:.3e}, |sum_a - 1| {colsum:.3e}, |sum_b - 1| {rowsum:.3e}")
        assert dev <= 1e-8 and colsum <= 1e-8 and rowsum <= 1e-8, (npt, dev, colsum, rowsum)


def test_orbital_weights_flat_and_degenerate_bands(abz):
    """The block-diagonal H = diag(e(k), e(k), 0.25) of test_ltm_flat_and_degenerate_bands_on_device."""
    so = orc.tb_integer(3)
    c = np.zeros((3, 3, 3, 3, 3), dtype=np.complex128)
    c[..., 0, 0] = so.c[..., 0, 0]
    c[..., 1, 1] = so.c[..., 0, 0]
    c[1, 1, 1, 2, 2] = 0.25
    s = abz.FourierSeries(c, period=1.0, first=(-1, -1, -1), ndim=3)
    rule = abz.DeviceRule(s.device(), 8, None, abz._lib.WANT_EIG)
    W = device_weights(rule)
    rule.close()
    assert np.abs(W.sum(axis=2) - 1.0).max() <= 1e-8 and np.abs(W.sum(axis=0) - 1.0).max() <= 1e-8


# ---------------------------------------------------------------- 4. the scan reads what the kernel wrote
@pytest.mark.parametrize("name", ["svo", "syn6"])
def test_weighted_scan_of_device_weights(abz, name):
    s, npt = make_case(abz, name)
    assert npt == (20 if name == "svo" else 12)
    rule = abz.DeviceRule(s.device(), npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    W = device_weights(rule)
    lists = energy_lists(eig, np.random.default_rng(5))
    worst = 0.0
    for label in ("seven", "linspace300"):
        Es = lists[label]
        g_ref, N_ref = wn.wltm(eig, on_grid(rule, W), Es)
        worst = max(worst, check(rule.ltm(Es, elements="attached"), g_ref, f"device weights {name} {label} g"))
        worst = max(worst, check(rule.ltm(Es, states=True, elements="attached"), N_ref, f"device weights {name} {label} N"))
    rule.close()
    print(f"scan of device weights {name}: worst deviation / bound = {worst:.3e}")


# ---------------------------------------------------------------- 5. end to end
def test_projected_dos_with_device_eigenvectors(abz):
    s, npt = make_case(abz, "syn6")
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    eig = ln.rule_eigenvalues(s.device().rule(npt, None, abz._lib.WANT_EIG))
    Es = np.linspace(eig.min() - 0.1, eig.max() + 0.1, 61)
    plain = abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=npt)).u
    sol = abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=npt, elements="orbitals", eigenvectors="device"))
    assert sol.u.shape == (len(Es), 6) and sol.retcode
    check(sol.u.sum(axis=1), plain, "sum of the projected DOS")
    assert np.all(sol.u >= -1e-9 * max(1.0, plain.max()))
    one = abz.dos.solve(abz.DOSProblem(s, float(Es[30]), bz), abz.LTM(npt=npt, elements="orbitals", eigenvectors="device")).u
    assert one.shape == (6,)
    check(one, sol.u[30], "scalar domain")
    # the host route: the weights differ by at most 1e-10 (no close levels on this grid), and the corner weights of the
    # uncorrected tetrahedron DOS are non-negative: |dg_a| <= max|dW| g
    host = abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=npt, elements="orbitals")).u
    dev = np.abs(sol.u - host).max()
    bound = 1e-10 * max(1.0, plain.max()) + close(sol.u, host)[1]
    print(f"projected DOS, device against host eigenvectors: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound
    two = abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=npt, elements="orbitals", eigenvectors="device", orbitals=[0, 2])).u
    assert two.shape == (len(Es), 2)
    check(two, sol.u[:, [0, 2]], "orbitals=[0, 2]")
    N = abz.dos.solve(abz.DOSProblem(s, [eig.max() + 1.0], bz), abz.LTM(npt=npt, cumulative=True, elements="orbitals", eigenvectors="device")).u
    check(N[0], np.ones(6), "every orbital holds one state")


def test_device_orbitals_cache_follows_the_series(abz):
    so = orc.synthetic_wannier(3, rmax=2, seed=7)
    h = product_series(abz, so)
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    alg = abz.LTM(npt=10, elements="orbitals", eigenvectors="device")
    eig = ln.rule_eigenvalues(h.device().rule(10, None, abz._lib.WANT_EIG))
    Es = np.linspace(eig.min(), eig.max(), 11)[1:-1]
    cache = abz.dos.init(abz.DOSProblem(h, Es, bz), alg)
    u1 = abz.dos.solve_(cache).u
    check(u1, abz.dos.solve(abz.DOSProblem(product_series(abz, so), Es, bz), alg).u, "cache 1")
    assert np.array_equal(abz.dos.solve_(cache).u, u1)  # the weights stay attached
    h.c[...] = h.c * 0.5
    h.c[2, 2, 2, 0, 0] += 0.3  # the orbitals are no longer equivalent
    cache.isfresh = True
    u2 = abz.dos.solve_(cache).u
    fresh = abz.FourierSeries(h.c.copy(), period=1.0, first=so.first, ndim=3)
    check(u2, abz.dos.solve(abz.DOSProblem(fresh, Es, bz), alg).u, "cache 2")
    assert np.abs(u2 - u1).max() > 1e-3 and not cache.isfresh
    # another cache on the same rule attaches its own selection; this one attaches again
    other = abz.dos.init(abz.DOSProblem(h, Es, bz), abz.LTM(npt=10, elements="orbitals", eigenvectors="device", orbitals=[1]))
    if other.cacheval is cache.cacheval:
        check(abz.dos.solve_(other).u, u2[:, [1]], "second cache")
        check(abz.dos.solve_(cache).u, u2, "first cache again")


# ---------------------------------------------------------------- 6. export, refusals, bookkeeping
def test_elements_export_returns_what_was_attached(abz):
    L = abz._lib
    s, npt = make_case(abz, "svo")
    rule = abz.DeviceRule(s.device(), 9, None, L.WANT_EIG)
    assert rule.ltm_elements_export() is None
    A = np.random.default_rng(3).standard_normal((5, rule.nk, 3))
    rule.ltm_elements(A)
    assert np.array_equal(rule.ltm_elements_export(), A)
    nc = C.c_int(-1)
    assert L.lib().abz_rule_ltm_elements_export(rule.h, C.byref(nc), None) == 0 and nc.value == 5
    rule.ltm_elements(A[:1])
    assert np.array_equal(rule.ltm_elements_export(), A[:1])
    rule.ltm_elements(None)
    assert rule.ltm_elements_export() is None
    rule.ltm_elements(A)
    rule.rebuild()
    assert rule.ltm_elements_export() is None
    assert L.lib().abz_rule_ltm_elements_export(rule.h, None, None) == L.ERR_ARG
    rule.close()


def test_orbital_weights_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s = product_series(abz, orc.synthetic_wannier(3, rmax=2, seed=7))
    dev = s.device()
    orb = np.array([0, 1, 2, 0] * 5, dtype=np.int32)
    porb = orb.ctypes.data_as(L.c_i32p)

    def refused(rc, code, words=None):
        assert rc == code, (rc, code, lib.abz_last_error())
        assert len(lib.abz_last_error()) > 0
        if words is not None:
            assert words in lib.abz_last_error(), lib.abz_last_error()

    # rules that are not a whole periodic grid, or hold no eigenvalues
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, 8, cub.syms, L.WANT_EIG)
    refused(lib.abz_rule_ltm_orbitals(sym._h, None, 0), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, 8, 2, 6, L.WANT_EIG, C.byref(slab)))
    refused(lib.abz_rule_ltm_orbitals(slab, None, 0), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    assert lib.abz_rule_destroy(slab) == 0
    honly = abz.DeviceRule(dev, 8, None, L.WANT_H)
    refused(lib.abz_rule_ltm_orbitals(honly._h, None, 0), L.ERR_ARG)
    honly.close()

    def keeps(rule, A, rc, code, words=None):
        refused(rc, code, words)
        assert np.array_equal(rule.ltm_elements_export(), A)

    # an unfolded rule takes elements, not orbital weights
    unf = sym.unfold()
    A = np.random.default_rng(1).standard_normal((2, unf.nk, 3))
    unf.ltm_elements(A)
    keeps(unf, A, lib.abz_rule_ltm_orbitals(unf.h, None, 0), L.ERR_UNSUPPORTED, b"unfolded")
    unf.close()
    sym.close()
    # argument checks on a rule that qualifies
    full = abz.DeviceRule(dev, 8, None, L.WANT_EIG)
    A = np.random.default_rng(2).standard_normal((2, full.nk, 3))
    full.ltm_elements(A)
    h = full.h
    keeps(full, A, lib.abz_rule_ltm_orbitals(h, porb, 0), L.ERR_ARG)
    keeps(full, A, lib.abz_rule_ltm_orbitals(h, porb, -1), L.ERR_ARG)
    keeps(full, A, lib.abz_rule_ltm_orbitals(h, porb, 17), L.ERR_ARG)
    for bad in (3, -1, 1 << 20):
        o = np.array([0, bad, 1], dtype=np.int32)
        keeps(full, A, lib.abz_rule_ltm_orbitals(h, o.ctypes.data_as(L.c_i32p), 3), L.ERR_ARG)
    with pytest.raises(ValueError):
        full.ltm_orbitals([0, 3])
    with pytest.raises(ValueError):
        full.ltm_orbitals([0.5])
    assert np.array_equal(full.ltm_elements_export(), A) and full._ltm_ncomp == 2
    # valid calls afterwards: duplicates and sixteen components are fine
    assert lib.abz_rule_ltm_orbitals(h, porb, 16) == 0
    full._ltm_ncomp = 16
    W16 = full.ltm_elements_export()
    full.ltm_orbitals()
    assert np.array_equal(W16, full.ltm_elements_export()[orb[:16]])
    full.close()
    # band counts: NULL needs n <= 16; above 32 bands there is no kernel
    for n, o, no, code in ((17, None, 0, L.ERR_ARG), (33, porb, 3, L.ERR_UNSUPPORTED), (33, None, 0, L.ERR_UNSUPPORTED)):
        sn = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
        rule = abz.DeviceRule(sn.device(), 5, None, L.WANT_EIG)
        A = np.ones((1, rule.nk, n))
        rule.ltm_elements(A)
        keeps(rule, A, lib.abz_rule_ltm_orbitals(rule.h, o, no), code)
        rule.close()
    # a series that is not Hermitian
    c, first = rand_series(np.random.default_rng(9), (3, 3, 3), 3, hermitian=False)
    rule = abz.DeviceRule(abz.FourierSeries(c, period=1.0, first=first).device(), 5, None, L.WANT_H | L.WANT_EIG)
    A = np.ones((1, rule.nk, 3))
    rule.ltm_elements(A)
    keeps(rule, A, lib.abz_rule_ltm_orbitals(rule.h, None, 0), L.ERR_ARG, b"Hermitian")
    rule.close()
    # the Python mirror keeps the refusal of a k-sharded rule
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        r = dev.rule(8, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_orbitals()
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_elements_export()
    finally:
        dev.kshard, dev.allreduce = None, None


def test_orbital_weights_are_accounted(abz):
    """abz_mem_info: a call on a rule of eigenvalues only builds and destroys its transient H rule -- what stays is the
    element block."""
    L = abz._lib
    s, _ = make_case(abz, "syn6")
    dev = s.device()
    npt, n = 12, 6
    info = lambda: (dev.ctx.mem_info()[0], dev.ctx.mem_info()[4])

    def cycle():
        rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
        m1 = info()
        rule.ltm_elements(np.ones((n, rule.nk, n)))
        mh = info()
        rule.ltm_elements(None)
        rule.ltm_orbitals()
        m2 = info()
        rule.ltm_orbitals()  # replaces the block
        m2b = info()
        rule.ltm_orbitals([1, 4])
        m2c = info()
        rule.ltm_elements(None)
        m3 = info()
        rule.close()
        return m1, mh, m2, m2b, m2c, m3

    gc.collect()
    gc.disable()
    try:
        cycle()  # the context's and the series' scratch buffers grow once
        m1, mh, m2, m2b, m2c, m3 = cycle()
    finally:
        gc.enable()
    print(f"mem (bytes, blocks): rule {m1}, host elements {mh}, device weights {m2}, again {m2b}, two orbitals {m2c}, dropped {m3}")
    # one block more, of the element block's size (the caching allocator hands out a recycled block of up to twice the bytes
    # asked for, + 4 KB); nothing of the transient rule stays
    row = (npt + 15) // 16 * 16
    for m, ncomp in ((mh, n), (m2, n), (m2b, n), (m2c, 2)):
        size = 8 * ncomp * n * row * npt ** 2
        assert m[1] == m1[1] + 1 and size <= m[0] - m1[0] <= 2 * size + 4096, (m, m1, size)
    assert m3 == m1


def test_orbital_weights_profiling_slot(abz):
    L = abz._lib
    s, _ = make_case(abz, "syn6")
    dev = s.device()
    rules = [abz.DeviceRule(dev, 12, None, want) for want in (L.WANT_EIG, L.WANT_H | L.WANT_EIG)]
    dev.ctx.prof_enable(True, kernels=[L.K_EIG])
    try:
        for rule in rules:
            dev.ctx.prof_reset()
            rule.ltm_orbitals()
            ms, launches = dev.ctx.prof_read(L.K_EIG)
            assert launches >= 1 and ms > 0.0
            rule.ltm_orbitals([3])
            assert dev.ctx.prof_read(L.K_EIG)[1] >= launches + 1
    finally:
        dev.ctx.prof_enable(False)
        for rule in rules:
            rule.close()

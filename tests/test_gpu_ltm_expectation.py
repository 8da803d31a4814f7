"""Band expectation values q_i = Re u_b^H Hermitian(O_i(k)) u_b of operator series, and products of two of them, computed on the
device as matrix elements of the tetrahedron method (abz_rule_ltm_expectation, kernels_ltm_expect.hip), and the routes above
it (DeviceRule.ltm_expectation, LTM(elements=BandExpectation(...)), LTM(elements="velocities")), against LAPACK on exported
planes (tests/expect_numpy.py), independent device paths (eigenvalues, orbital weights, the GGR velocities) and the geometric
restatement of the weighted scan (tests/wltm_numpy.py, tests/gwltm_numpy.py).

Bounds.  Separated bands: the orbital tests' bound carries over -- the eigenvector error is about n eps ||H|| / gap, 1e-12 on
these models -- so a single expectation gets 1e-10 max(1, max_k ||O(k)||) and a product 1e-10 max(1, max||O_i|| max||O_j||).
Degenerate levels: any orthonormal basis of the eigenspace is an answer, so only sums of single expectations over a level are
compared, to 1e-8 of the same scale, the project's bound for eigenvector-derived sums.  Scans: the restatement is fed exported
device values, so the bound is the LTM parity bound 1e-9 max(1, max|ref|)."""
import ctypes as C

import numpy as np
import pytest

import abz_oracle as orc
import expect_numpy as xn
import gwltm_numpy as gw
import ltm_numpy as ln
import wltm_numpy as wn
from test_gpu_ltm import close, product_series
from test_gpu_ltm_weighted import check, on_grid
from test_gpu_parity import rand_series

pytestmark = pytest.mark.gpu

MIXED = [0, (1, -1), (2, 2), (0, 1), 2, (0, 1)]  # singles, a square, a cross product, duplicates


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def operator_series(abz, n, nops, dims, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nops):
        c, first = rand_series(rng, dims, n, hermitian=True)
        out.append(abz.FourierSeries(c, period=1.0, first=first, ndim=len(dims)))
    return out


def exported_h(abz, series, npt):
    rule = abz.DeviceRule(series.device(), npt, None, abz._lib.WANT_H)
    try:
        return rule.export(x=False, w=False, H=True)["H"]
    finally:
        rule.close()


def attached(rule, ops, comps=None):
    rule.ltm_expectation(ops, comps)
    A = rule.ltm_elements_export()
    ncomp = len(ops) if comps is None else len(comps)
    assert rule._ltm_ncomp == ncomp and A.shape == (ncomp, rule.nk, rule.dev.s.n) and np.all(np.isfinite(A))
    return A


def check_against_numpy(abz, s, ops, npt, comps, what, want=None):
    L = abz._lib
    rule = abz.DeviceRule(s.device(), npt, None, L.WANT_H | L.WANT_EIG if want is None else want)
    try:
        H = exported_h(abz, s, npt)
        O = [exported_h(abz, o, npt) for o in ops]
        ref, bound = xn.elements(H, O, comps), xn.bounds(O, comps)
        A = attached(rule, ops, comps)
        dev = np.abs(A - ref).max(axis=(1, 2))
        print(f"expectations {what} npt={npt} nops={len(ops)} ncomp={len(A)}: max dev / bound {np.max(dev / bound):.3e} (max||O|| {max(xn.norms(O)):.2f})")
        assert np.all(dev <= bound), (what, npt, dev, bound)
    finally:
        rule.close()


# ---------------------------------------------------------------- 1. against numpy: band counts, grids, operator counts
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 16, 17, 24])
def test_expectations_match_lapack(abz, n):
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    ops = operator_series(abz, n, 8, (3, 3, 3), 1000 + n)
    for npt in (5, 12):
        check_against_numpy(abz, s, ops[:3], npt, MIXED, f"syn{n}")
    check_against_numpy(abz, s, ops[:1], 5, None, f"syn{n} one operator")
    sixteen = [(i % 8, -1) for i in range(8)] + [(i, (3 * i + 1) % 8) for i in range(8)]
    check_against_numpy(abz, s, ops, 5, sixteen, f"syn{n} eight operators")


# ---------------------------------------------------------------- 2. lower dimensions, one band
@pytest.mark.parametrize("d,dims,npts", [(1, (5,), (9, 40)), (2, (3, 5), (7,))])
def test_expectations_in_one_and_two_dimensions(abz, d, dims, npts):
    """40 points of a 6-band line are two passes of 32 nodes; 9 and 7 leave most of the last pass empty."""
    c, first = rand_series(np.random.default_rng(100 * d + 6), dims, 6, hermitian=True)
    s = abz.FourierSeries(c, period=1.0, first=first, ndim=d)
    ops = operator_series(abz, 6, 3, dims, 50 + d)
    for npt in npts:
        check_against_numpy(abz, s, ops, npt, MIXED, f"{d}-D 6 bands")


def test_expectation_of_a_scalar_series_is_the_operator(abz):
    L = abz._lib
    s = product_series(abz, orc.tb_integer(2))
    (o,) = operator_series(abz, 1, 1, (3, 3), 12)
    O = np.real(xn.matrices(exported_h(abz, o, 9)))[:, 0, 0]
    for want in (L.WANT_EIG, L.WANT_H | L.WANT_EIG):
        rule = abz.DeviceRule(s.device(), 9, None, want)
        A = attached(rule, [o], [0, (0, 0)])
        rule.close()
        assert A.shape == (2, 81, 1) and np.array_equal(A[0, :, 0], O) and np.array_equal(A[1, :, 0], O * O)


# ---------------------------------------------------------------- 3. layouts
@pytest.mark.parametrize("n", [3, 6, 12, 17])
def test_expectations_do_not_depend_on_the_plane_layouts(abz, n):
    L = abz._lib
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    ops = operator_series(abz, n, 3, (3, 3, 3), 30 + n)
    npt, blocks = 12, []
    ref, bound = None, None
    for owant in (L.WANT_H, L.WANT_H | L.WANT_H_COMPACT):
        orules = [abz.DeviceRule(o.device(), npt, None, owant) for o in ops]
        # the library built the layout asked for; above 16 bands there is no compact layout and it drops the bit (abzhip.h)
        assert all(r.want == (owant if n <= 16 else L.WANT_H) for r in orules)
        if ref is None:
            O = [r.export(x=False, w=False, H=True)["H"] for r in orules]
            ref, bound = xn.elements(exported_h(abz, s, npt), O, MIXED), xn.bounds(O, MIXED)
        for want in (L.WANT_EIG, L.WANT_H | L.WANT_EIG, L.WANT_H | L.WANT_EIG | L.WANT_H_COMPACT):
            rule = abz.DeviceRule(s.device(), npt, None, want)
            A = attached(rule, orules, MIXED)
            assert np.array_equal(A, attached(rule, orules, MIXED)), (owant, want)  # two calls on one rule
            blocks.append(A)
            rule.close()
        for r in orules:
            r.close()
    assert np.all(np.abs(blocks[0] - ref).max(axis=(1, 2)) <= bound)
    assert all(np.array_equal(blocks[0], b) for b in blocks[1:])


# ---------------------------------------------------------------- 4. independent device paths
@pytest.mark.parametrize("n", [3, 12])
def test_expectation_of_h_is_the_eigenvalue(abz, n):
    """O = H (ops = {r}): q_b = e_b, and the scan of the attached block is the scan of the energy."""
    L = abz._lib
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    rule = abz.DeviceRule(s.device(), 12, None, L.WANT_H | L.WANT_EIG)
    ex = rule.export(x=False, w=False, H=True, eig=True)
    A = attached(rule, [rule])
    bound = 1e-10 * max(1.0, np.linalg.norm(ex["H"], 2, axis=(1, 2)).max())
    dev = np.abs(A[0] - ex["eig"]).max()
    print(f"<H> against the eigenvalues, {n} bands: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound
    Es = np.linspace(ex["eig"].min() - 0.1, ex["eig"].max() + 0.1, 41)
    for states in (False, True):
        check(rule.ltm(Es, states=states, elements="attached"), rule.ltm(Es, states=states, elements="energy"), f"<H> scan states={states}")
    rule.close()


@pytest.mark.parametrize("n", [3, 12])
def test_expectation_of_an_orbital_projector_is_the_orbital_weight(abz, n):
    """O = |a><a|, one coefficient at R = 0: q_b = |U_ab|^2, the block of abz_rule_ltm_orbitals."""
    L = abz._lib
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    orbs = [n - 1, 0, 1]
    ops = []
    for a in orbs:
        c = np.zeros((1, 1, 1, n, n), dtype=np.complex128)
        c[0, 0, 0, a, a] = 1.0
        ops.append(abz.FourierSeries(c, period=1.0, first=(0, 0, 0), ndim=3))
    rule = abz.DeviceRule(s.device(), 12, None, L.WANT_EIG)
    A = attached(rule, ops)
    rule.ltm_orbitals(orbs)
    W = rule.ltm_elements_export()
    rule.close()
    dev = np.abs(A - W).max()
    print(f"<|a><a|> against the orbital weights, {n} bands: max dev {dev:.3e} (bound 1.0e-10)")
    assert dev <= 1e-10


@pytest.mark.parametrize("n", [3, 12])
def test_expectation_of_the_derivative_is_the_band_velocity(abz, n):
    """O_j = h.derivative(j) against the velocity planes of a WANT_EIG | WANT_VEL rule: the fused GGR kernel (3 bands) and the
    rows kernel (12 bands), which evaluate dH/dk_j from the coefficients themselves.  Bound relative to max|v|."""
    L = abz._lib
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    vrule = abz.DeviceRule(s.device(), 12, None, L.WANT_EIG | L.WANT_VEL)
    vel = vrule.export(x=False, w=False, vel=True)["vel"].transpose(1, 0, 2)  # [d, nk, n]
    vrule.close()
    rule = abz.DeviceRule(s.device(), 12, None, L.WANT_EIG)
    A = attached(rule, [s.derivative(j) for j in range(3)])
    rule.close()
    dev, bound = np.abs(A - vel).max(), 1e-10 * max(1.0, np.abs(vel).max())
    print(f"<dH/dk> against the GGR velocities, {n} bands: max dev {dev:.3e} (bound {bound:.1e}, max|v| {np.abs(vel).max():.3f})")
    assert dev <= bound


# ---------------------------------------------------------------- 5. degenerate levels
@pytest.mark.parametrize("n3,mult", [(3, 2), (2, 4), (3, 3), (4, 4)])
def test_expectations_of_degenerate_levels(abz, n3, mult):
    """H = Q (I_mult x h(k)) Q^H, every level `mult` times (test_orbital_weights_of_degenerate_levels): sums of the single
    expectations over each level against LAPACK's."""
    L = abz._lib
    rng = np.random.default_rng(7 * n3 + mult)
    c3, first = rand_series(rng, (3, 3, 3), n3, hermitian=True)
    n = n3 * mult
    q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    c = np.einsum("ab,...bc,dc->...ad", q, np.kron(np.eye(mult), c3), q.conj())
    c = 0.5 * (c + np.conj(np.swapaxes(c[::-1, ::-1, ::-1], -1, -2)))  # exactly Hermitian; the levels stay degenerate to rounding
    s = abz.FourierSeries(c, period=1.0, first=first)
    ops = operator_series(abz, n, 3, (3, 3, 3), 70 + n)
    for npt in (5, 19):
        rule = abz.DeviceRule(s.device(), npt, None, L.WANT_H | L.WANT_EIG)
        ex = rule.export(x=False, w=False, H=True, eig=True)
        e = ex["eig"]
        A = attached(rule, ops)
        rule.close()
        O = [exported_h(abz, o, npt) for o in ops]
        scale = np.abs(e).max()
        e3 = e.reshape(len(e), n3, mult)[:, :, 0]
        sep = np.min(np.diff(e3, axis=1), axis=1) > 1e-6 * scale
        assert sep.mean() > 0.9
        got = xn.cluster_sums(e[sep], A[:, sep], 1e-6 * scale)
        ref = xn.cluster_sums(e[sep], xn.expectations(ex["H"][sep], [o[sep] for o in O]), 1e-6 * scale)
        dev, bound = np.abs(got - ref).max(axis=(1, 2)), xn.bounds(O, None, rel=1e-8)
        print(f"degenerate levels {n3} x {mult} npt={npt}: level sums, max dev / bound {np.max(dev / bound):.3e}")
        assert np.all(dev <= bound), (npt, dev, bound)


# ---------------------------------------------------------------- 6. through dos
def velocity_reference(abz, h, npt):
    """(eig on the grid, v_a v_b elements [d (d + 1) / 2] on the grid) from a WANT_EIG | WANT_VEL rule's exports."""
    L = abz._lib
    d = h.d
    rule = abz.DeviceRule(h.device(), npt, None, L.WANT_EIG | L.WANT_VEL)
    ex = rule.export(x=False, w=False, eig=True, vel=True)
    eig = ln.rule_eigenvalues(rule)
    v = ex["vel"].transpose(1, 0, 2)
    A = on_grid(rule, np.stack([v[a] * v[b] for a in range(d) for b in range(a, d)]))
    rule.close()
    return eig, A


def test_transport_distribution_through_dos(abz):
    so = orc.synthetic_wannier(3, rmax=2, seed=7)
    h = product_series(abz, so)
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    npt = 10
    eig, A = velocity_reference(abz, h, npt)
    Es = np.linspace(eig.min() - 0.1, eig.max() + 0.1, 31)
    g_ref, N_ref = wn.wltm(eig, A, Es)
    sol = abz.dos.solve(abz.DOSProblem(h, Es, bz), abz.LTM(npt=npt, elements="velocities"))
    assert sol.u.shape == (len(Es), 6) and sol.retcode
    check(sol.u, g_ref, "transport distribution")
    assert np.all(sol.u[:, [0, 3, 5]] >= -1e-9 * max(1.0, np.abs(g_ref).max()))  # the diagonal is a sum of squares
    check(abz.dos.solve(abz.DOSProblem(h, Es, bz), abz.LTM(npt=npt, elements="velocities", cumulative=True)).u, N_ref, "its integral")
    one = abz.dos.solve(abz.DOSProblem(h, float(Es[12]), bz), abz.LTM(npt=npt, elements="velocities")).u
    assert one.shape == (6,)
    check(one, g_ref[12], "scalar domain")
    eta = 0.05
    G = gw.green_weighted(eig, A, Es + 1j * eta)
    check(abz.dos.solve(abz.DOSProblem(h, Es, bz), abz.LTM(npt=npt, elements="velocities", eta=eta)).u, -G.imag / np.pi, "broadened")
    # the same through a BandExpectation of the derivative series
    be = abz.BandExpectation(abz.velocity_operators(h), [(a, b) for a in range(3) for b in range(a, 3)])
    check(abz.dos.solve(abz.DOSProblem(h, Es, bz), abz.LTM(npt=npt, elements=be)).u, g_ref, "BandExpectation")
    # node weights contracted with the attached block against the scan of it
    mid = Es[11:19]  # inside the bands before and after the change below
    cache = abz.dos.init(abz.DOSProblem(h, mid, bz), abz.LTM(npt=npt, elements="velocities", cumulative=True))
    u = abz.dos.solve_(cache).u
    cache.cacheval.ltm_node_weights(mid, states=True, export=False)
    check(cache.cacheval.ltm_node_weights_dot(), u, "node weights dot")
    # the cache follows the series
    h.c[...] = h.c * 0.5
    h.c[2, 2, 2, 0, 0] += 0.3
    cache.H = h
    u2 = abz.dos.solve_(cache).u
    fresh = abz.FourierSeries(h.c.copy(), period=1.0, first=so.first, ndim=3)
    eig2, A2 = velocity_reference(abz, fresh, npt)
    N2 = wn.wltm(eig2, A2, mid)[1]
    check(u2, N2, "after the series changed")
    assert np.abs(u2 - u).max() > 1e-3 and np.abs(N2).min() > 1e-3 and not cache.isfresh


def test_transport_integral_of_a_cosine_band_on_the_device(abz):
    """e = -2 cos 2 pi kappa: the device's N_A of v^2 within 1e-9 of the restatement fed the closed-form e and v at the nodes
    (test_ltm_expectation_cpu compares the restatement with the exact integral)."""
    h = abz.FourierSeries(np.array([-1.0, 0.0, -1.0]), period=1.0, first=-1)
    bz = abz.load_bz(abz.FBZ(), [[2 * np.pi]])
    Es = np.array([-1.5, -0.7, 0.0, 0.3, 1.1, 1.5, 2.5])
    for npt in (100, 400):
        kappa = np.arange(npt) / npt
        eig = (-2 * np.cos(2 * np.pi * kappa)).reshape(npt, 1)
        v2 = ((4 * np.pi * np.sin(2 * np.pi * kappa)) ** 2).reshape(npt, 1)
        u = abz.dos.solve(abz.DOSProblem(h, Es, bz), abz.LTM(npt=npt, elements="velocities", cumulative=True)).u
        assert u.shape == (len(Es), 1)
        check(u, wn.wltm(eig, v2, Es)[1], f"cosine band npt={npt}")


# ---------------------------------------------------------------- 7. refusals
def test_expectation_refusals(abz):
    L = abz._lib
    lib = L.lib()
    n = 3
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    (o,) = operator_series(abz, n, 1, (3, 3, 3), 5)
    dev, odev = s.device(), o.device()
    oh = abz.DeviceRule(odev, 8, None, L.WANT_H)
    comps = np.array([[0, -1], [0, 0]] * 10, dtype=np.int32)
    pc = comps.ctypes.data_as(L.c_i32p)

    def handles(*rules):
        """Operator handles as the C array: DeviceRules, raw handles or None (a NULL entry)."""
        raw = [r.h if isinstance(r, abz.DeviceRule) else r for r in rules]
        return (C.c_void_p * len(rules))(*[getattr(r, "value", r) for r in raw])

    def refused(rc, code, words=None):
        assert rc == code, (rc, code, lib.abz_last_error())
        assert len(lib.abz_last_error()) > 0
        if words is not None:
            assert words in lib.abz_last_error(), lib.abz_last_error()

    # target rules that are not a whole periodic grid, or hold no eigenvalues
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, 8, cub.syms, L.WANT_EIG)
    refused(lib.abz_rule_ltm_expectation(sym._h, handles(oh), 1, None, 0), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, 8, 2, 6, L.WANT_EIG, C.byref(slab)))
    refused(lib.abz_rule_ltm_expectation(slab, handles(oh), 1, None, 0), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    assert lib.abz_rule_destroy(slab) == 0
    honly = abz.DeviceRule(dev, 8, None, L.WANT_H)
    refused(lib.abz_rule_ltm_expectation(honly._h, handles(oh), 1, None, 0), L.ERR_ARG)

    def keeps(rule, A, rc, code, words=None):
        refused(rc, code, words)
        assert np.array_equal(rule.ltm_elements_export(), A)

    unf = sym.unfold()
    A = np.random.default_rng(1).standard_normal((2, unf.nk, n))
    unf.ltm_elements(A)
    keeps(unf, A, lib.abz_rule_ltm_expectation(unf.h, handles(oh), 1, None, 0), L.ERR_UNSUPPORTED, b"unfolded")
    unf.close()
    # argument checks on a rule that qualifies
    full = abz.DeviceRule(dev, 8, None, L.WANT_EIG)
    A = np.random.default_rng(2).standard_normal((2, full.nk, n))
    full.ltm_elements(A)
    h = full.h
    keeps(full, A, lib.abz_rule_ltm_expectation(h, None, 1, None, 0), L.ERR_ARG)
    keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(None), 1, None, 0), L.ERR_ARG)
    keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(oh, None), 2, None, 0), L.ERR_ARG)
    for nops in (0, -1, 9):
        keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(*[oh] * 9), nops, None, 0), L.ERR_ARG)
    for ncomp in (0, -1, 17):
        keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(oh), 1, pc, ncomp), L.ERR_ARG)
    for bad in ((1, -1), (-1, -1), (0, 1), (0, -2), (1 << 20, 0)):
        cb = np.array([[0, -1], bad], dtype=np.int32)
        keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(oh), 1, cb.ctypes.data_as(L.c_i32p), 2), L.ERR_ARG)
    # operators: another grid, another band count, another dimension, another context, no H planes, a slab, irreducible nodes,
    # a series that is not Hermitian
    other = abz.DeviceRule(odev, 6, None, L.WANT_H)
    keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(other), 1, None, 0), L.ERR_ARG)
    other.close()
    (o4,) = operator_series(abz, 4, 1, (3, 3, 3), 6)
    r4 = abz.DeviceRule(o4.device(), 8, None, L.WANT_H)
    keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(r4), 1, None, 0), L.ERR_ARG)
    r4.close()
    (o2,) = operator_series(abz, n, 1, (3, 3), 7)
    r2 = abz.DeviceRule(o2.device(), 8, None, L.WANT_H)
    keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(r2), 1, None, 0), L.ERR_ARG)
    r2.close()
    ctx2 = L.Context()
    rc2 = abz.DeviceRule(o.device(ctx2), 8, None, L.WANT_H)
    keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(rc2), 1, None, 0), L.ERR_ARG, b"context")
    rc2.close()
    eonly = abz.DeviceRule(odev, 8, None, L.WANT_EIG)
    keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(eonly), 1, None, 0), L.ERR_ARG, b"no H planes")
    keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(full), 1, None, 0), L.ERR_ARG, b"no H planes")  # ops = {r} needs r's H
    eonly.close()
    orm = C.c_void_p()  # a rule asked for with the row-major bit of abz_eval_nodes
    L.check(lib.abz_ptr_rule_build(odev.h, 8, 0, None, None, L.WANT_H | L.WANT_H_ROW_MAJOR, C.byref(orm)))
    keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(orm), 1, None, 0), L.ERR_UNSUPPORTED, b"row-major")
    assert lib.abz_rule_destroy(orm) == 0
    oslab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(odev.h, 8, 2, 6, L.WANT_H, C.byref(oslab)))
    keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(oslab), 1, None, 0), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    assert lib.abz_rule_destroy(oslab) == 0
    osym = abz.DeviceRule(odev, 8, cub.syms, L.WANT_H)
    keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(osym._h), 1, None, 0), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    osym.close()
    cn, fn = rand_series(np.random.default_rng(9), (3, 3, 3), n, hermitian=False)
    rn = abz.DeviceRule(abz.FourierSeries(cn, period=1.0, first=fn).device(), 8, None, L.WANT_H | L.WANT_EIG)
    keeps(full, A, lib.abz_rule_ltm_expectation(h, handles(rn), 1, None, 0), L.ERR_ARG, b"Hermitian")
    An = np.ones((1, rn.nk, n))
    rn.ltm_elements(An)
    keeps(rn, An, lib.abz_rule_ltm_expectation(rn.h, handles(oh), 1, None, 0), L.ERR_ARG, b"Hermitian")  # ... nor the target's
    rn.close()
    # the Python mirror refuses before the library is called
    for bad in ([], [o] * 9, [3.0]):
        with pytest.raises(ValueError):
            full.ltm_expectation(bad)
    with pytest.raises(ValueError):
        full.ltm_expectation([o], [(0, 1)])
    with pytest.raises(ValueError):
        full.ltm_expectation([o], [0] * 17)
    assert np.array_equal(full.ltm_elements_export(), A) and full._ltm_ncomp == 2
    # valid calls afterwards: duplicates and sixteen components are fine
    assert lib.abz_rule_ltm_expectation(h, handles(oh, oh), 2, pc, 16) == 0
    full._ltm_ncomp = 16
    A16 = full.ltm_elements_export()
    q = attached(full, [oh])
    assert np.array_equal(A16[0], q[0]) and np.array_equal(A16[1], q[0] * q[0]) and np.array_equal(A16[14], A16[0])
    full.close()
    sym.close()
    honly.close()
    # more than 32 bands
    s33 = product_series(abz, orc.synthetic_wannier(33, rmax=2, seed=7))
    r33 = abz.DeviceRule(s33.device(), 5, None, L.WANT_H | L.WANT_EIG)
    A33 = np.ones((1, r33.nk, 33))
    r33.ltm_elements(A33)
    keeps(r33, A33, lib.abz_rule_ltm_expectation(r33.h, handles(r33), 1, None, 0), L.ERR_UNSUPPORTED, b"33 bands")
    r33.close()
    oh.close()
    # a k-sharded rule, and a k-sharded series through dos
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        r = dev.rule(8, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_expectation([o])
        bz = abz.load_bz(abz.FBZ(), np.eye(3))
        for el in ("velocities", abz.BandExpectation([o])):
            with pytest.raises(NotImplementedError, match="k-sharded"):
                abz.dos.init(abz.DOSProblem(s, [0.0], bz), abz.LTM(npt=8, elements=el))
    finally:
        dev.kshard, dev.allreduce = None, None


def test_expectation_profiling_slot(abz):
    """The kernels are booked under ABZ_K_EIG, like the orbital kernels."""
    L = abz._lib
    for n in (3, 6):
        s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
        ops = operator_series(abz, n, 2, (3, 3, 3), 90 + n)
        dev = s.device()
        rule = abz.DeviceRule(dev, 8, None, L.WANT_H | L.WANT_EIG)
        orules = [o.device().rule(8, None, L.WANT_H) for o in ops]
        dev.ctx.prof_enable(True, kernels=[L.K_EIG])
        try:
            dev.ctx.prof_reset()
            rule.ltm_expectation(orules)
            ms, launches = dev.ctx.prof_read(L.K_EIG)
            assert launches >= 1 and ms > 0.0
        finally:
            dev.ctx.prof_enable(False)
            rule.close()

"""Pair rules of the tetrahedron method on the device (abz_rule_ltm_pairs, kernels_ltm_pairs.hip) and the routes above them
(DeviceRule.ltm_pairs, LTM(pairs=BandPairs(...)), abz.dos.joint_dos / interband): the pair energies bit for bit against the
source rule's eigenvalues, the interband products against LAPACK on exported planes (tests/pairs_numpy.py), every scan on the
pair rule against its geometric restatement, and two checks that use no restatement.

Bounds.  Energies: one subtraction, exact.  Elements on separated bands: 1e-10 max(1, max||O_i|| max||O_j||) per component, the
project's bound for products of eigenvector-derived quantities (expect_numpy.bounds).  Degenerate levels: sums over the pairs
between two levels, to 1e-8 of the same scale.  Scans: the restatement is fed exported device values, so the bound is the LTM
parity bound 1e-9 max(1, max|ref|)."""
import ctypes as C
import os

import numpy as np
import pytest

import abz_oracle as orc
import gltm_numpy as gn
import gnodew_numpy as gnw
import gwltm_numpy as gw
import ltm_numpy as ln
import nodew_numpy as nw
import pairs_numpy as pn
import wltm_numpy as wn
from test_gpu_ltm import close, product_series
from test_gpu_ltm_expectation import exported_h, operator_series
from test_gpu_parity import rand_series

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MIXED = [0, (0, 1), (1, 0, "im"), (2, 1, "re"), (1, 2, "im"), 2, (0, 1)]  # squares, cross products, both parts, a duplicate


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def check(u, ref, what):
    u, ref = np.asarray(u), np.asarray(ref)
    assert u.shape == ref.shape and np.all(np.isfinite(np.ascontiguousarray(u).view(np.float64))), (what, u.shape, ref.shape)
    if np.iscomplexobj(ref):
        dev = max(np.abs(u.real - ref.real).max(), np.abs(u.imag - ref.imag).max())
        bound = 1e-9 * max(1.0, np.abs(ref.real).max(), np.abs(ref.imag).max())
    else:
        dev, bound = close(u, ref)
    print(f"pairs {what}: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)


def on_grid(rule, A):
    """[.., nk, nb] -> [..] + [npt] * d + [nb]"""
    return A.reshape(A.shape[:-2] + (rule.npt,) * rule.dev.s.d + (A.shape[-1],))


def random_series(abz, n, dims, seed):
    c, first = rand_series(np.random.default_rng(seed), dims, n, hermitian=True)
    return abz.FourierSeries(c, period=1.0, first=first, ndim=len(dims))


# ---------------------------------------------------------------- 1. energies, bit for bit
def check_energies(src, lower, upper):
    eig = src.export(x=False, w=False, eig=True)["eig"]
    pr = src.ltm_pairs(lower, upper)
    try:
        (v0, nv), (c0, nc) = lower, upper
        assert pr.nbands == nv * nc and pr.nk == src.nk and pr._ltm_ncomp == 0 and pr.ltm_elements_export() is None
        D = pr.export(eig=True)
        assert D["eig"].shape == (src.nk, nv * nc)
        assert np.array_equal(D["eig"], pn.pair_energies(eig, v0, nv, c0, nc)), (lower, upper)
        full = src.export()
        assert np.array_equal(D["x"], full["x"]) and np.array_equal(D["w"], full["w"])
    finally:
        pr.close()


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 16, 24, 40])
def test_pair_energies_are_the_differences_of_the_source(abz, n):
    L = abz._lib
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    if n == 40:
        ranges = [((16, 8), (24, 8))]  # nops = 0 on the 33...64-band path of the scans' source, 64 pairs exactly
    else:
        ranges = [((0, 1), (n - 1, 1))]
        if n >= 4:
            ranges += [((0, 1), (1, n - 1)), ((0, n - 1), (n - 1, 1))]  # nv < nc, nv > nc
        if n >= 5:
            ranges += [((1, 1), (n - 3, 2))]  # an interior window, unused bands on both sides
        if n == 16:
            ranges += [((0, 8), (8, 8))]  # 64 pairs exactly
    for npt in (5, 12) if n < 24 else (5,):
        src = abz.DeviceRule(s.device(), npt, None, L.WANT_EIG)
        for lower, upper in ranges:
            check_energies(src, lower, upper)
        src.close()


@pytest.mark.parametrize("d,dims,npts", [(1, (5,), (9, 40)), (2, (3, 5), (7,))])
def test_pair_energies_in_one_and_two_dimensions(abz, d, dims, npts):
    s = random_series(abz, 6, dims, 100 * d + 6)
    for npt in npts:
        src = abz.DeviceRule(s.device(), npt, None, abz._lib.WANT_EIG)
        for lower, upper in [((0, 2), (3, 3)), ((1, 3), (4, 2))]:
            check_energies(src, lower, upper)
        src.close()


def test_pair_energies_of_an_unfolded_source(abz):
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))  # cubic: the 48 operations are symmetries of H
    cub = abz.load_bz(abz.CubicSymIBZ(), 3.85856 * np.eye(3))
    sym = abz.DeviceRule(s.device(), 8, cub.syms, abz._lib.WANT_EIG)
    unf = sym.unfold()
    check_energies(unf, (0, 1), (1, 2))
    check_energies(unf, (0, 2), (2, 1))
    with pytest.raises(abz._lib.AbzError, match="unfolded"):
        unf.ltm_pairs((0, 1), (1, 2), operator_series(abz, 3, 1, (3, 3, 3), 3))
    unf.close()
    sym.close()


# ---------------------------------------------------------------- 2. elements against LAPACK
def check_elements(abz, src, H, ops, O, lower, upper, comps, what):
    (v0, nv), (c0, nc) = lower, upper
    pr = src.ltm_pairs(lower, upper, ops, comps)
    try:
        A = pr.ltm_elements_export()
        ref, bound = pn.elements(H, O, v0, nv, c0, nc, comps), pn.bounds(O, comps)
        assert pr._ltm_ncomp == len(ref) and A.shape == ref.shape == (len(ref), src.nk, nv * nc) and np.all(np.isfinite(A))
        dev = np.abs(A - ref).max(axis=(1, 2))
        print(f"pair elements {what} npt={src.npt} {nv}x{nc} nops={len(ops)} ncomp={len(A)}: max dev / bound {np.max(dev / bound):.3e}")
        assert np.all(dev <= bound), (what, lower, upper, dev, bound)
        eig = src.export(x=False, w=False, eig=True)["eig"]
        assert np.array_equal(pr.export(x=False, w=False, eig=True)["eig"], pn.pair_energies(eig, v0, nv, c0, nc))
        return A
    finally:
        pr.close()


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 16, 17, 24, 32])
def test_pair_elements_match_lapack(abz, n):
    L = abz._lib
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    ops = operator_series(abz, n, 4, (3, 3, 3), 2000 + n)
    h = n // 2
    for npt in (5, 12):
        H = exported_h(abz, s, npt)
        O = [exported_h(abz, o, npt) for o in ops]
        for want in (L.WANT_EIG, L.WANT_H | L.WANT_EIG):  # H from a transient rule, and from the source's own planes
            src = abz.DeviceRule(s.device(), npt, None, want)
            if n == 2:
                check_elements(abz, src, H, ops[:3], O[:3], (0, 1), (1, 1), MIXED, "syn2")
            else:
                lo, up = (0, min(h - 1, 3)) if h > 1 else (0, 1), (h, min(n - h, 8))  # nv < nc: the lower range's u_v are parked
                check_elements(abz, src, H, ops[:3], O[:3], lo, up, MIXED, f"syn{n}")
                lo, up = (0, min(h + (n & 1), 8)), (n - max(1, min(h - 1, 3)), max(1, min(h - 1, 3)))  # nv > nc: the upper range's y_c
                check_elements(abz, src, H, ops[:3], O[:3], lo, up, MIXED, f"syn{n}")
            if want == L.WANT_EIG and npt == 5:
                lo, up = ((0, 1), (n - 1, 1)) if n < 5 else ((1, 1), (n - 3, 2))
                check_elements(abz, src, H, ops[:1], O[:1], lo, up, None, f"syn{n} one operator")
                four = [(i, j, part) for i in range(4) for j in range(i, 4) for part in ("re", "im")][:16]
                check_elements(abz, src, H, ops, O, lo, up, four, f"syn{n} four operators")
                check_elements(abz, src, H, ops, O, lo, up, None, f"syn{n} four operators, squares")
                if n in (16, 32):  # 64 pairs of 4 operators: the largest LDS tile
                    check_elements(abz, src, H, ops, O, (n // 2 - 8, 8), (n // 2, 8), four, f"syn{n} 8 x 8 pairs")
            src.close()


def device_block(abz, base, nbytes):
    """nbytes at the device address `base` as doubles (hipMemcpy of the HIP runtime the library is linked against)"""
    L = abz._lib
    buf = np.empty(nbytes // 8)
    memcpy = L.lib().hipMemcpy
    memcpy.restype, memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert memcpy(buf.ctypes.data, base, nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return buf


@pytest.mark.parametrize("n,npt,lower,upper", [(3, 5, (0, 1), (1, 2)), (4, 17, (0, 2), (2, 2)),       # one node per lane
                                               (6, 5, (0, 2), (3, 3)), (6, 40, (1, 3), (4, 2)),       # 8 lanes: one pass, two passes
                                               (12, 12, (2, 3), (6, 5)), (12, 20, (0, 6), (8, 2)),    # 16 lanes: one pass, two passes
                                               (20, 5, (0, 3), (10, 8)), (20, 12, (2, 8), (12, 3))])  # 32 lanes: one pass, two passes
def test_pair_elements_padding_columns_are_zero(abz, n, npt, lower, upper):
    """The resident element block through its device address (abz_rule_ltm_elements_ptr): columns npt .. row-1 of every plane
    hold exact zeros -- the lane kernels write them from their zeroed registers, the row kernels in the tail of the line's last
    pass -- and the other columns are what the export returns.  2-D grids: lines of up to 40 points at little cost."""
    L = abz._lib
    s = random_series(abz, n, (3, 3), 600 + n)
    ops = operator_series(abz, n, 2, (3, 3), 700 + n)
    row = (npt + 15) // 16 * 16
    src = abz.DeviceRule(s.device(), npt, None, L.WANT_EIG)
    comps = [0, (0, 1, "im"), 1]
    pr = src.ltm_pairs(lower, upper, ops, comps)
    nb = pr.nbands
    base, nbytes, ncomp = pr.ltm_elements_ptr()
    assert base and ncomp == 3 and nbytes == 8 * npt * 3 * nb * row
    blk = device_block(abz, base, nbytes).reshape(npt, 3, nb, row)
    assert np.all(blk[..., npt:] == 0.0)
    A = pr.ltm_elements_export()  # [ncomp, nk, nb]
    assert np.array_equal(blk[..., :npt].transpose(1, 0, 3, 2).reshape(3, npt * npt, nb), A) and np.abs(A).max() > 0.0
    assert src.ltm_elements_ptr() == (0, 0, 0)
    pr.ltm_elements(None)
    assert pr.ltm_elements_ptr() == (0, 0, 0)
    pr.close()
    src.close()


@pytest.mark.parametrize("n,npt,lower,upper", [(6, 40, (0, 2), (3, 3)), (8, 40, (0, 5), (5, 3)), (12, 20, (1, 3), (6, 6)), (16, 20, (0, 8), (8, 8)),
                                               (16, 36, (3, 6), (12, 2))])
def test_pair_elements_of_lines_of_several_passes(abz, n, npt, lower, upper):
    """Lines longer than the 32 (8 lanes per node) or 16 (16 lanes) nodes of one pass, against LAPACK: 2-D grids."""
    L = abz._lib
    s = random_series(abz, n, (3, 3), 800 + n)
    ops = operator_series(abz, n, 3, (3, 3), 900 + n)
    H = exported_h(abz, s, npt)
    O = [exported_h(abz, o, npt) for o in ops]
    src = abz.DeviceRule(s.device(), npt, None, L.WANT_EIG)
    check_elements(abz, src, H, ops, O, lower, upper, MIXED, f"2-D {n} bands")
    src.close()


def test_scans_on_a_rule_of_64_pairs(abz):
    """8 x 8 pairs of 16 bands: the JDOS and a two-component spectrum on all 64 pseudo-bands against the restatements."""
    s = product_series(abz, orc.synthetic_wannier(16, rmax=2, seed=7))
    ops = operator_series(abz, 16, 2, (3, 3, 3), 64)
    src = abz.DeviceRule(s.device(), 4, None, abz._lib.WANT_EIG)
    pr = src.ltm_pairs((0, 8), (8, 8), ops, [0, (0, 1, "im")])
    assert pr.nbands == 64
    D = on_grid(pr, pr.export(x=False, w=False, eig=True)["eig"])
    A = on_grid(pr, pr.ltm_elements_export())
    ws = np.linspace(D.min() - 0.05, D.max() + 0.05, 9)
    g, N = ln.ltm(D, ws)
    check(pr.ltm(ws), g, "JDOS of 64 pairs")
    check(pr.ltm(ws, states=True), N, "cumulative JDOS of 64 pairs")
    gA, NA = wn.wltm(D, A, ws)
    check(pr.ltm(ws, elements="attached"), gA, "spectra of 64 pairs")
    check(pr.ltm(ws, states=True, elements="attached"), NA, "cumulative spectra of 64 pairs")
    zs = ws[2:7:2] + 0.05j
    check(pr.ltm_green(zs, elements="attached"), gw.green_weighted(D, A, zs), "G_A of 64 pairs")
    pr.close()
    src.close()


def test_pair_energy_padding_columns_are_zero(abz):
    """The resident energy planes through their device address: columns npt .. row-1 of every plane hold exact zeros, whatever
    the padding of the source's planes holds."""
    L = abz._lib
    for n, lower, upper in ((3, (0, 1), (1, 2)), (6, (0, 2), (3, 3))):
        s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
        ops = operator_series(abz, n, 2, (3, 3, 3), 40 + n)
        npt, row = 5, 16
        src = abz.DeviceRule(s.device(), npt, None, L.WANT_EIG)
        pr = src.ltm_pairs(lower, upper, ops, [0, (0, 1, "im"), 1])
        nb = pr.nbands
        base, nbytes = pr.values_ptr()
        assert nbytes == 8 * npt * npt * nb * row
        buf = np.empty(nbytes // 8)
        memcpy = L.lib().hipMemcpy  # (the HIP runtime the library is linked against)
        memcpy.restype, memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert memcpy(buf.ctypes.data, base, nbytes, 2) == 0  # hipMemcpyDeviceToHost
        E = buf.reshape(npt * npt, nb, row)
        assert np.all(E[:, :, npt:] == 0.0) and np.all(E[:, :, :npt] > 0.0)
        assert np.array_equal(E[:, :, :npt].transpose(0, 2, 1).reshape(-1, nb), pr.export(x=False, w=False, eig=True)["eig"])
        pr.close()
        src.close()


# ---------------------------------------------------------------- 3. degenerate levels
@pytest.mark.parametrize("n3,mult", [(2, 2), (3, 2), (3, 3)])
def test_pair_elements_of_degenerate_levels(abz, n3, mult):
    """H = Q (I_mult x h(k)) Q^H, every level `mult` times (test_expectations_of_degenerate_levels): the lowest level against
    all others, sums over the pairs between two levels against LAPACK's."""
    L = abz._lib
    rng = np.random.default_rng(7 * n3 + mult)
    c3, first = rand_series(rng, (3, 3, 3), n3, hermitian=True)
    n = n3 * mult
    q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    c = np.einsum("ab,...bc,dc->...ad", q, np.kron(np.eye(mult), c3), q.conj())
    c = 0.5 * (c + np.conj(np.swapaxes(c[::-1, ::-1, ::-1], -1, -2)))  # exactly Hermitian; the levels stay degenerate to rounding
    s = abz.FourierSeries(c, period=1.0, first=first)
    ops = operator_series(abz, n, 2, (3, 3, 3), 70 + n)
    comps = [0, (0, 1), (0, 1, "im"), 1]
    lower, upper = (0, mult), (mult, n - mult)
    npt = 7
    src = abz.DeviceRule(s.device(), npt, None, L.WANT_H | L.WANT_EIG)
    ex = src.export(x=False, w=False, H=True, eig=True)
    e = ex["eig"]
    pr = src.ltm_pairs(lower, upper, ops, comps)
    A = pr.ltm_elements_export()
    pr.close()
    src.close()
    O = [exported_h(abz, o, npt) for o in ops]
    scale = np.abs(e).max()
    e3 = e.reshape(len(e), n3, mult)[:, :, 0]
    sep = np.min(np.diff(e3, axis=1), axis=1) > 1e-6 * scale
    assert sep.mean() > 0.9
    args = lower + upper + (1e-6 * scale,)
    got = pn.level_pair_sums(e[sep], A[:, sep], *args)
    ref = pn.level_pair_sums(e[sep], pn.elements(ex["H"][sep], [o[sep] for o in O], *lower, *upper, comps), *args)
    dev, bound = np.abs(got - ref).max(axis=(1, 2)), pn.bounds(O, comps, rel=1e-8)
    print(f"degenerate levels {n3} x {mult}: level-pair sums, max dev / bound {np.max(dev / bound):.3e}")
    assert np.all(dev <= bound), (dev, bound)


# ---------------------------------------------------------------- 4. scans on the pair rule
@pytest.fixture(scope="module")
def scanned(abz):
    """One pair rule with elements (6 bands, 2 x 3 pairs, npt 6) and its exported energies and elements on the grid."""
    s = product_series(abz, orc.synthetic_wannier(6, rmax=2, seed=7))
    ops = operator_series(abz, 6, 2, (3, 3, 3), 77)
    src = abz.DeviceRule(s.device(), 6, None, abz._lib.WANT_EIG)
    pr = src.ltm_pairs((1, 2), (3, 3), ops, [0, (0, 1), (0, 1, "im")])
    D = on_grid(pr, pr.export(x=False, w=False, eig=True)["eig"])
    A = on_grid(pr, pr.ltm_elements_export())
    ws = np.linspace(D.min() - 0.05, D.max() + 0.05, 13)
    zs = np.concatenate([ws[2:9:2] + 0.05j, [ws[5] - 0.2j, ws[0] - 1.0 + 1e-3j]])
    yield pr, D, A, ws, zs
    pr.close()
    src.close()


def test_ltm_on_a_pair_rule(scanned):
    pr, D, A, ws, _ = scanned
    g, N = ln.ltm(D, ws)
    check(pr.ltm(ws), g, "JDOS")
    check(pr.ltm(ws, states=True), N, "cumulative JDOS")
    assert abs(pr.ltm(ws[-1:], states=True)[0] - 6.0) <= 1e-9 * 6 and pr.ltm(ws[:1], states=True)[0] == 0.0  # the six pairs


def test_weighted_ltm_on_a_pair_rule(scanned):
    import bloechl_numpy as bn
    pr, D, A, ws, _ = scanned
    g, N = wn.wltm(D, A, ws)
    check(pr.ltm(ws, elements="attached"), g, "spectra")
    check(pr.ltm(ws, states=True, elements="attached"), N, "cumulative spectra")
    corr = bn.correction(D, A, ws)
    check(pr.ltm(ws, states=True, elements="attached", correction=True), N + corr, "Bloechl-corrected")
    ge, Ne = wn.wltm(D, D[None], ws)
    check(pr.ltm(ws, elements="energy"), ge, "energy-weighted")


def test_green_on_a_pair_rule(scanned):
    pr, D, A, _, zs = scanned
    check(pr.ltm_green(zs), gn.green_trace(D, zs), "tr G")
    check(pr.ltm_green(zs, elements="attached"), gw.green_weighted(D, A, zs), "G_A")


def test_node_weights_on_a_pair_rule(scanned):
    pr, D, A, ws, zs = scanned
    Es = ws[3:9:2]
    W = pr.ltm_node_weights(Es, states=True)
    assert W.shape == (len(Es), pr.nk, 6)
    ref = nw.node_weights(D, Es, "states").reshape(W.shape)
    check(pr.nk * W, pr.nk * ref, "node weights (nk w)")
    check(pr.ltm_node_weights_dot(), pr.ltm(Es, states=True, elements="attached"), "node weights dot")
    Wz = pr.ltm_green_node_weights(zs[:3])
    assert Wz.shape == (3, pr.nk, 6)
    check(pr.nk * Wz, pr.nk * gnw.node_weights(D, zs[:3]).reshape(Wz.shape), "complex node weights (nk W)")
    check(pr.ltm_green_node_weights_dot(), pr.ltm_green(zs[:3], elements="attached"), "complex node weights dot")
    assert pr.ltm_node_weights_ptr()[1] == 8 * 36 * len(Es) * 6 * 16 and pr.ltm_green_node_weights_ptr()[1] == 8 * 36 * 2 * 3 * 6 * 16


# ---------------------------------------------------------------- 5. two checks that do not use the restatement
def test_jdos_of_a_diagonal_two_band_model_is_the_dos_of_one_band(abz):
    """H = diag(-eps, eps), eps = a + b cos 2 pi k > 0: the pair energy is 2 eps, and the JDOS is the one-band ltm of the series
    2 eps on the same grid."""
    L = abz._lib
    a, b, npt = 1.5, 0.7, 40
    c = np.zeros((3, 2, 2), dtype=np.complex128)
    c[1] = np.diag([-a, a])
    c[0] = c[2] = np.diag([-b / 2, b / 2])
    two = abz.FourierSeries(c, period=1.0, first=-1, ndim=1)
    one = abz.FourierSeries(np.array([b, 2 * a, b]), period=1.0, first=-1)
    src = abz.DeviceRule(two.device(), npt, None, L.WANT_EIG)
    ref = abz.DeviceRule(one.device(), npt, None, L.WANT_EIG)
    pr = src.ltm_pairs(range(0, 1), range(1, 2))
    ws = np.linspace(2 * (a - b) - 0.1, 2 * (a + b) + 0.1, 37)
    scale = np.abs(pr.export(eig=True)["eig"] - ref.export(eig=True)["eig"]).max()
    for states in (False, True):
        u, r = pr.ltm(ws, states=states), ref.ltm(ws, states=states)
        dev, bound = np.abs(u - r).max(), 1e-12 * max(1.0, np.abs(r).max())
        print(f"diagonal two-band model {'N' if states else 'J'}: max dev {dev:.3e} (bound {bound:.1e}; energies differ by {scale:.1e})")
        assert dev <= bound
    for r in (pr, src, ref):
        r.close()


def test_cumulative_spectrum_above_all_pairs_is_the_grid_mean(abz):
    L = abz._lib
    for n, lower, upper in ((3, (0, 1), (1, 2)), (9, (1, 3), (5, 4))):
        s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
        ops = operator_series(abz, n, 2, (3, 3, 3), 500 + n)
        src = abz.DeviceRule(s.device(), 6, None, L.WANT_EIG)
        pr = src.ltm_pairs(lower, upper, ops, [0, (0, 1), (0, 1, "im"), 1])
        A = pr.ltm_elements_export()
        top = pr.export(eig=True)["eig"].max() + 1.0
        N = pr.ltm([top], states=True, elements="attached")[0]
        mean = A.sum(axis=2).mean(axis=1)
        scale = np.abs(A).sum(axis=2).mean(axis=1).max()
        dev = np.abs(N - mean).max()
        print(f"N_A above all pairs, {n} bands: max dev {dev:.3e} (bound {1e-12 * scale:.1e})")
        assert dev <= 1e-12 * scale
        pr.close()
        src.close()


# ---------------------------------------------------------------- 6. top level
def svo(abz):
    return abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))


def test_interband_spectrum_through_dos(abz):
    L = abz._lib
    h = svo(abz)
    bz = abz.load_bz(abz.FBZ(), 3.85856 * np.eye(3))
    npt = 12
    src = h.device().rule(npt, None, L.WANT_EIG)
    comps = [(a, b, "re") for a in range(3) for b in range(a, 3)]
    low = src.ltm_pairs((0, 1), (1, 2), abz.velocity_operators(h), comps)
    D = low.export(eig=True)["eig"]
    ws = np.linspace(D.min() - 0.02, D.max() + 0.02, 21)
    ref = low.ltm(ws, elements="attached")
    alg = abz.LTM(npt=npt, pairs=abz.BandPairs(nocc=1, operators="velocities"))
    sol = abz.dos.solve(abz.DOSProblem(h, ws, bz), alg)
    assert sol.u.shape == (len(ws), 6) and sol.retcode and np.array_equal(sol.u, ref)
    assert np.all(sol.u[:, [0, 3, 5]] >= 0.0) and sol.u[:, [0, 3, 5]].max() > 0.0  # sums of |M|^2
    assert np.array_equal(abz.dos.interband(abz.DOSProblem(h, None, bz), ws, nocc=1, npt=npt), ref)
    one = abz.dos.solve(abz.DOSProblem(h, float(ws[9]), bz), alg).u
    assert one.shape == (6,) and np.array_equal(one, low.ltm(ws[9:10], elements="attached")[0])  # (the scan of one energy)
    check(one, ref[9], "scalar domain")
    Nref = low.ltm(ws, states=True, elements="attached")
    cum = abz.LTM(npt=npt, cumulative=True, pairs=abz.BandPairs(nocc=1, operators="velocities"))
    assert np.array_equal(abz.dos.solve(abz.DOSProblem(h, ws, bz), cum).u, Nref)
    cor = abz.LTM(npt=npt, cumulative=True, correction=True, pairs=abz.BandPairs(lower=(0, 1), upper=range(1, 3), operators="velocities"))
    assert np.array_equal(abz.dos.solve(abz.DOSProblem(h, ws, bz), cor).u, low.ltm(ws, states=True, elements="attached", correction=True))
    # JDOS
    jd = abz.dos.solve(abz.DOSProblem(h, ws, bz), abz.LTM(npt=npt, pairs=abz.BandPairs(nocc=1))).u
    assert jd.shape == (len(ws),) and np.array_equal(jd, low.ltm(ws)) and np.array_equal(abz.dos.joint_dos(abz.DOSProblem(h, None, bz), ws, nocc=1, npt=npt), jd)
    # eta: complex, -Im / pi the broadened spectrum; over all w it integrates to the cumulative value above all pairs.  The map
    # w = w0 + s tan(theta) makes the integrand a smooth pi-periodic function of theta: the midpoint rule converges geometrically
    eta = 0.5 * (D.max() - D.min())
    m = 128
    theta = (np.arange(m) + 0.5) * np.pi / m - np.pi / 2
    w0, sc = 0.5 * (D.max() + D.min()), eta
    wq = w0 + sc * np.tan(theta)
    G = abz.dos.solve(abz.DOSProblem(h, wq, bz), abz.LTM(npt=npt, eta=eta, pairs=abz.BandPairs(nocc=1, operators="velocities"))).u
    assert G.dtype == np.complex128 and G.shape == (m, 6)
    assert np.array_equal(G, low.ltm_green(wq + 1j * eta, elements="attached"))
    integral = ((-G.imag / np.pi) * (sc / np.cos(theta) ** 2)[:, None]).sum(axis=0) * (np.pi / m)
    total = low.ltm([D.max() + 1.0], states=True, elements="attached")[0]
    check(integral, total, "integral of the broadened spectrum")
    assert np.abs(G.real).max() > 0.0
    assert np.array_equal(abz.dos.interband(abz.DOSProblem(h, None, bz), wq[:8] + 1j * eta, nocc=1, npt=npt), G[:8])
    low.close()


def test_joint_dos_from_irreducible_nodes(abz):
    h = svo(abz)
    cub = abz.load_bz(abz.CubicSymIBZ(), 3.85856 * np.eye(3))
    ws = np.linspace(0.05, 1.2, 24)  # (not w = 0: the t2g bands touch at high-symmetry points, where J(0) hangs on the last bit)
    full = abz.dos.joint_dos(abz.DOSProblem(h, None, cub), ws, nocc=1, npt=12)
    sym = abz.dos.joint_dos(abz.DOSProblem(h, None, cub), ws, nocc=1, npt=12, symmetric=True)
    assert full.max() > 0.0
    check(sym, full, "JDOS from irreducible nodes")
    cache = abz.dos.init(abz.DOSProblem(h, ws, cub), abz.LTM(npt=12, symmetric=True, pairs=abz.BandPairs(nocc=1)))
    assert isinstance(cache.cacheval, abz.series.PairRule) and isinstance(cache.cacheval.source, abz.UnfoldedRule)
    assert np.array_equal(abz.dos.solve_(cache).u, sym) and np.array_equal(abz.dos.joint_dos(cache, ws), sym)


def test_pair_cache_follows_the_series(abz):
    so = orc.synthetic_wannier(3, rmax=2, seed=7)
    h = product_series(abz, so)
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    alg = abz.LTM(npt=8, cumulative=True, pairs=abz.BandPairs(nocc=1, operators="velocities"))
    ws = np.array([0.5, 1.0, 2.0, 50.0])
    cache = abz.dos.init(abz.DOSProblem(h, ws, bz), alg)
    u = abz.dos.solve_(cache).u
    rule = cache.cacheval
    h.c[...] = h.c * 0.5
    h.c[2, 2, 2, 0, 0] += 0.3
    cache.H = h
    u2 = abz.dos.solve_(cache).u
    assert cache.cacheval is rule and not cache.isfresh  # filled again in place
    fresh = abz.FourierSeries(h.c.copy(), period=1.0, first=so.first, ndim=3)
    assert np.array_equal(u2, abz.dos.solve(abz.DOSProblem(fresh, ws, bz), alg).u)
    assert np.abs(u2 - u).max() > 1e-3


# ---------------------------------------------------------------- 7. hygiene
def test_two_calls_and_a_refill_write_the_same_bits(abz):
    L = abz._lib
    for n, lower, upper in ((3, (0, 1), (1, 2)), (12, (2, 4), (6, 5))):
        so = orc.synthetic_wannier(n, rmax=2, seed=7)
        s = product_series(abz, so)
        ops = operator_series(abz, n, 3, (3, 3, 3), 300 + n)
        src = abz.DeviceRule(s.device(), 7, None, L.WANT_EIG)
        a, b = src.ltm_pairs(lower, upper, ops, MIXED), src.ltm_pairs(lower, upper, ops, MIXED)
        Aa = a.ltm_elements_export()
        assert np.array_equal(Aa, b.ltm_elements_export()) and np.array_equal(a.export(eig=True)["eig"], b.export(eig=True)["eig"])
        b.close()
        a.ltm_node_weights([0.5], export=False)
        a.ltm_green_node_weights([0.5 + 0.1j], export=False)
        h0 = a.h.value
        a.refill()
        assert a.h.value == h0 and np.array_equal(a.ltm_elements_export(), Aa)
        assert a.ltm_node_weights_ptr() == (0, 0, 0) and a.ltm_green_node_weights_ptr() == (0, 0, 0)  # stale weight blocks are gone
        # new coefficients: the refilled rule is a fresh pair rule of the new series, bit for bit
        a.ltm_node_weights([0.5], export=False)
        Ea = a.export(eig=True)["eig"]
        s.c[...] = s.c * 0.75
        s.c[2, 2, 2, 0, 0] += 0.3  # (a scaled H alone keeps its eigenvectors, and with them the elements)
        s.invalidate()
        Ab, Eb = a.ltm_elements_export(), a.export(eig=True)["eig"]  # (a.h refills: source first, then the pair rule)
        assert a.h.value == h0 and a.ltm_node_weights_ptr() == (0, 0, 0)
        s2 = abz.FourierSeries(s.c.copy(), period=1.0, first=so.first, ndim=3)
        src2 = abz.DeviceRule(s2.device(), 7, None, L.WANT_EIG)
        f = src2.ltm_pairs(lower, upper, ops, MIXED)
        assert np.array_equal(Ab, f.ltm_elements_export()) and np.array_equal(Eb, f.export(eig=True)["eig"])
        assert np.abs(Ab - Aa).max() > 1e-6 and np.abs(Eb - Ea).max() > 1e-6
        for r in (f, src2, a, src):
            r.close()


def test_making_a_pair_rule_leaves_the_source_alone(abz):
    L = abz._lib
    n = 6
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    ops = operator_series(abz, n, 2, (3, 3, 3), 9)
    src = abz.DeviceRule(s.device(), 6, None, L.WANT_H | L.WANT_EIG)
    A = np.random.default_rng(3).standard_normal((2, src.nk, n))
    src.ltm_elements(A)
    Es = np.linspace(-1.0, 1.0, 5)
    before = (src.ltm(Es), src.ltm(Es, elements="attached"), src.ltm_node_weights(Es[:2]), src.ltm_green_node_weights([0.1 + 0.2j]),
              src.export(H=True, eig=True))
    dots = (src.ltm_node_weights_dot(), src.ltm_green_node_weights_dot())
    wp, gp = src.ltm_node_weights_ptr(), src.ltm_green_node_weights_ptr()
    pr = src.ltm_pairs((0, 2), (3, 3), ops)
    pr.ltm_node_weights([1.0], export=False)
    assert src.ltm_node_weights_ptr() == wp and src.ltm_green_node_weights_ptr() == gp and src._ltm_ncomp == 2
    assert np.array_equal(src.ltm_elements_export(), A)
    assert np.array_equal(src.ltm(Es), before[0]) and np.array_equal(src.ltm(Es, elements="attached"), before[1])
    assert np.array_equal(src.ltm_node_weights_dot(), dots[0]) and np.array_equal(src.ltm_green_node_weights_dot(), dots[1])
    after = src.export(H=True, eig=True)
    assert all(np.array_equal(after[k], before[4][k]) for k in after)
    src.close()  # the pair rule does not depend on its source afterwards
    assert pr.ltm([1.0]).shape == (1,) and pr.ltm_elements_export().shape == (2, 216, 6)
    pr.close()


def test_pair_rule_refusals(abz):
    L = abz._lib
    lib = L.lib()
    n = 6
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    (o,) = operator_series(abz, n, 1, (3, 3, 3), 5)
    dev, odev = s.device(), o.device()
    oh = abz.DeviceRule(odev, 6, None, L.WANT_H)
    src = abz.DeviceRule(dev, 6, None, L.WANT_EIG)
    A = np.random.default_rng(2).standard_normal((2, src.nk, n))
    src.ltm_elements(A)

    def handles(*rules):
        raw = [r.h if isinstance(r, abz.DeviceRule) else r for r in rules]
        return (C.c_void_p * len(rules))(*[getattr(r, "value", r) for r in raw])

    def call(srch, v0, nv, c0, nc, ops=(), nops=None, comps=None, ncomp=0, out=None):
        box = C.c_void_p(out)
        pc = None if comps is None else np.ascontiguousarray(comps, dtype=np.int32).ctypes.data_as(L.c_i32p)
        rc = lib.abz_rule_ltm_pairs(srch, v0, nv, c0, nc, handles(*ops) if ops else None, len(ops) if nops is None else nops, pc, ncomp, C.byref(box))
        return rc, box.value

    def refused(got, code, words=None, out=None):
        rc, box = got
        assert rc == code and box == out, (rc, code, lib.abz_last_error())
        assert len(lib.abz_last_error()) > 0
        if words is not None:
            assert words in lib.abz_last_error(), lib.abz_last_error()
        assert np.array_equal(src.ltm_elements_export(), A)

    h = src.h
    # ranges
    for v0, nv, c0, nc in ((-1, 1, 1, 1), (0, 0, 1, 1), (0, 1, 1, 0), (0, 2, 1, 2), (2, 1, 0, 1), (0, 1, 5, 2), (0, 1, 6, 1), (0, 1, 1, -1)):
        refused(call(h, v0, nv, c0, nc), L.ERR_ARG)
        refused(call(h, v0, nv, c0, nc, [oh]), L.ERR_ARG)
    s40 = product_series(abz, orc.synthetic_wannier(40, rmax=2, seed=7))
    r40 = abz.DeviceRule(s40.device(), 5, None, L.WANT_EIG)
    rc, box = call(r40.h, 0, 9, 9, 8)
    assert rc == L.ERR_ARG and box is None and b"window" in lib.abz_last_error()
    rc, box = call(r40.h, 0, 2, 2, 2, [r40])
    assert rc == L.ERR_UNSUPPORTED and box is None and b"40 bands" in lib.abz_last_error()
    r40.close()
    # operators and components
    refused(call(h, 0, 1, 1, 1, [oh], nops=5), L.ERR_ARG)
    refused(call(h, 0, 1, 1, 1, [oh], nops=-1), L.ERR_ARG)
    refused((lib.abz_rule_ltm_pairs(h, 0, 1, 1, 1, None, 1, None, 0, C.byref(C.c_void_p())), None), L.ERR_ARG)
    refused((lib.abz_rule_ltm_pairs(h, 0, 1, 1, 1, None, 0, None, 0, None), None), L.ERR_ARG)
    refused(call(h, 0, 1, 1, 1, [None]), L.ERR_ARG)
    for ncomp in (0, -1, 17):
        refused(call(h, 0, 1, 1, 1, [oh], comps=[[0, 0, 0]] * 17, ncomp=ncomp), L.ERR_ARG)
    for bad in ((1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, 0, 2), (0, 0, -1)):
        refused(call(h, 0, 1, 1, 1, [oh], comps=[[0, 0, 0], bad], ncomp=2), L.ERR_ARG)
    eonly = abz.DeviceRule(odev, 6, None, L.WANT_EIG)
    refused(call(h, 0, 1, 1, 1, [eonly]), L.ERR_ARG, b"no H planes")
    eonly.close()
    other = abz.DeviceRule(odev, 5, None, L.WANT_H)
    refused(call(h, 0, 1, 1, 1, [other]), L.ERR_ARG)
    other.close()
    oslab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(odev.h, 6, 2, 4, L.WANT_H, C.byref(oslab)))
    refused(call(h, 0, 1, 1, 1, [oslab]), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    assert lib.abz_rule_destroy(oslab) == 0
    # sources that are not a whole periodic grid
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, 6, 2, 4, L.WANT_EIG, C.byref(slab)))
    for ops in ((), (oh,)):
        rc, box = call(slab, 0, 1, 1, 1, ops)
        assert rc == L.ERR_UNSUPPORTED and box is None and b"not a whole periodic grid" in lib.abz_last_error()
    assert lib.abz_rule_destroy(slab) == 0
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, 6, cub.syms, L.WANT_EIG)
    rc, box = call(sym._h, 0, 1, 1, 1)
    assert rc == L.ERR_UNSUPPORTED and box is None
    sym.close()
    honly = abz.DeviceRule(dev, 6, None, L.WANT_H)
    rc, box = call(honly._h, 0, 1, 1, 1)
    assert rc == L.ERR_ARG and box is None
    honly.close()
    # a pair rule: what it refuses, and what a refusal leaves
    pr = src.ltm_pairs((0, 2), (3, 3), [oh], [0, (0, 0, "im")])
    P, D = pr.ltm_elements_export(), pr.export(eig=True)["eig"]
    assert np.all(P[1] == 0.0)  # Im |M|^2
    pr.ltm_node_weights([1.0], export=False)
    wp = pr.ltm_node_weights_ptr()
    ph = pr.h
    nb = C.c_int(0)
    assert lib.abz_rule_ltm_bands(ph, C.byref(nb)) == 0 and nb.value == 6 == pr.nbands and src.nbands == n
    assert lib.abz_rule_ltm_bands(ph, None) == L.ERR_ARG
    out = np.zeros(4096)
    po = out.ctypes.data_as(L.c_f64p)
    orb = np.zeros(1, dtype=np.int32)
    z = np.array([0.5, 0.1])
    pairs_rc = [
        lib.abz_rule_ltm_orbitals(ph, None, 0), lib.abz_rule_ltm_orbitals(ph, orb.ctypes.data_as(L.c_i32p), 1),
        lib.abz_rule_ltm_projectors(ph, np.zeros(2, dtype=np.int32).ctypes.data_as(L.c_i32p), 1),
        lib.abz_rule_ltm_expectation(ph, handles(oh), 1, None, 0),
        lib.abz_rule_ltm_density_matrix(ph, po), lib.abz_rule_ltm_green_node_weights_matrix(ph, po),
        lib.abz_rule_ltm_halo(ph), lib.abz_rule_rebuild(ph),
        lib.abz_rule_reduce(ph, L.F_DOS_EIG, z.ctypes.data_as(L.c_f64p), 1, z.ctypes.data_as(L.c_f64p), 1, 1, po),
        call(ph, 0, 1, 1, 1)[0], call(ph, 0, 1, 1, 1, [oh])[0],
    ]
    for rc in pairs_rc:
        assert rc == L.ERR_UNSUPPORTED, (pairs_rc, lib.abz_last_error())
    assert b"pair rule" in lib.abz_last_error()
    # *out that does not match: another range, other components, another source geometry, not a pair rule
    for args in ((0, 2, 3, 2, [oh], None, [[0, 0, 0], [0, 0, 1]], 2), (0, 2, 3, 3, [oh], None, [[0, 0, 0], [0, 0, 0]], 2), (0, 2, 3, 3, [oh], None, None, 0),
                 (0, 2, 3, 3, (), None, None, 0)):
        refused(call(h, *args, out=ph.value), L.ERR_ARG, out=ph.value)
    refused(call(h, 0, 2, 3, 3, [oh], None, [[0, 0, 0], [0, 0, 1]], 2, out=h.value), L.ERR_ARG, b"not a rule made by", out=h.value)
    refused(call(h, 0, 2, 3, 3, [oh], None, [[0, 0, 0], [0, 0, 2]], 2, out=ph.value), L.ERR_ARG, out=ph.value)
    assert np.array_equal(pr.ltm_elements_export(), P) and np.array_equal(pr.export(eig=True)["eig"], D) and pr.ltm_node_weights_ptr() == wp
    for name in ("ltm_orbitals", "ltm_density_matrix"):
        with pytest.raises(L.AbzError, match="pair rule"):
            getattr(pr, name)()
    with pytest.raises(L.AbzError, match="pair rule"):
        pr.ltm_pairs((0, 1), (1, 1))
    # the Python mirror refuses before the library is called
    for bad in (((0, 2), (1, 2)), ((0, 1), (6, 1)), (range(0, 4, 2), (5, 1)), ((0, 1), 3)):
        with pytest.raises(ValueError):
            src.ltm_pairs(*bad)
    with pytest.raises(ValueError):
        src.ltm_pairs((0, 1), (1, 1), [o] * 5)
    with pytest.raises(ValueError):
        src.ltm_pairs((0, 1), (1, 1), [o], [(0, 1)])
    with pytest.raises(ValueError):
        src.ltm_pairs((0, 1), (1, 1), None, [0])
    assert np.array_equal(src.ltm_elements_export(), A)
    pr.close()
    oh.close()
    src.close()
    # a k-sharded rule, and a k-sharded series through dos
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        r = dev.rule(6, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError):
            r.ltm_pairs((0, 1), (1, 1))
        bz = abz.load_bz(abz.FBZ(), np.eye(3))
        for bp in (abz.BandPairs(nocc=2), abz.BandPairs(nocc=2, operators="velocities")):
            with pytest.raises(NotImplementedError, match="k-sharded"):
                abz.dos.init(abz.DOSProblem(s, [0.0], bz), abz.LTM(npt=6, pairs=bp))
    finally:
        dev.kshard, dev.allreduce = None, None


def test_pair_rule_memory_books(abz):
    """abz_mem_info returns to its starting value once the pair rules are closed (convention of test_gpu_mem_books.py); the second
    round: the context's scratch and the series' pools have their size by then."""
    L = abz._lib
    n = 6
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    ops = operator_series(abz, n, 2, (3, 3, 3), 9)
    dev = s.device()
    src = abz.DeviceRule(dev, 6, None, L.WANT_EIG)
    orules = [abz.DeviceRule(o.device(), 6, None, L.WANT_H) for o in ops]

    def books():
        info = dev.ctx.mem_info()
        return info[0], info[4]

    def round_trip():
        a = src.ltm_pairs((0, 2), (3, 3), orules, [0, (0, 1)])
        b = src.ltm_pairs((0, 2), (3, 3))
        a.ltm([1.0], elements="attached")
        a.ltm_node_weights([1.0], export=False)
        a.ltm_green_node_weights([1.0 + 0.1j], export=False)
        a.refill()
        held = books()
        a.close()
        b.close()
        return held

    round_trip()
    start = books()
    held = round_trip()
    assert held[0] >= start[0] + 8 * 216 * 6 * (1 + 2 + 1) and held[1] >= start[1] + 3
    assert books() == start
    for r in orules + [src]:
        r.close()


def test_pair_rule_profiling_slots(abz):
    """The element kernels are booked under ABZ_K_EIG, the energies under ABZ_K_LTM."""
    L = abz._lib
    for n in (3, 6):
        s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
        ops = operator_series(abz, n, 2, (3, 3, 3), 90 + n)
        dev = s.device()
        src = abz.DeviceRule(dev, 8, None, L.WANT_H | L.WANT_EIG)
        orules = [o.device().rule(8, None, L.WANT_H) for o in ops]
        dev.ctx.prof_enable(True, kernels=[L.K_EIG, L.K_LTM])
        try:
            dev.ctx.prof_reset()
            pr = src.ltm_pairs((0, 1), (1, n - 1), orules)
            for k in (L.K_EIG, L.K_LTM):
                ms, launches = dev.ctx.prof_read(k)
                assert launches >= 1 and ms > 0.0
            pr.close()
        finally:
            dev.ctx.prof_enable(False)
        src.close()

"""Interband spectra of metals on the device (abz_rule_ltm_pairs_occupied, ltm_pairs_occ_kernel of kernels_ltm_pairs_occ.hip) and the
routes above it (PairRule.ltm_occupied, abz.dos.joint_dos / interband with fermi= / nstates=).

Parity: against the geometric restatement tests/pairs_occ_numpy.py fed exported device eigenvalues and elements, to the LTM parity
bound of test_gpu_ltm_pairs.py, 1e-9 max(1, max|ref|).  The inputs are CASES of test_ltm_pairs_occupied_cpu.py, whose seeds and Fermi
levels were picked on the CPU so that every cut case occurs and no edge that E_F cuts is shorter than 1e-6 (a shorter one would ask
for another seed, not for a wider bound: d1_npt9 took seed 10 and the 3-d cases the seeds 1, 4, 1, 8, 7 after the first ones tried
missed cut cases).  Checks that need no restatement: the three identities of the CPU file on the device, degenerate bands, ties,
refusals and the dos routes."""
import ctypes as C
import os

import numpy as np
import pytest

import abz_oracle as orc
import ltm_numpy as ln
import pairs_occ_numpy as po
from test_gpu_ltm import close, product_series
from test_gpu_parity import rand_series
from test_ltm_pairs_occupied_cpu import CASES, case_oracle_series

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def check(u, ref, what):
    u, ref = np.asarray(u), np.asarray(ref)
    assert u.shape == ref.shape and np.all(np.isfinite(u)), (what, u.shape, ref.shape)
    dev, bound = close(u, ref)
    print(f"pairs occupied {what}: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)


def on_grid(rule, A):
    """[.., nk, nb] -> [..] + [npt] * d + [nb]"""
    return A.reshape(A.shape[:-2] + (rule.npt,) * rule.dev.s.d + (A.shape[-1],))


def svo(abz):
    return abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))


def energy_lists(D, rng):
    """a coarse equispaced list (the index of a window by arithmetic) and a fine irregular one (by search), both a little wider
    than the pair energies"""
    lo, hi = D.min() - 0.05 * (D.max() - D.min()) - 0.01, D.max() + 0.05 * (D.max() - D.min()) + 0.01
    return np.linspace(lo, hi, 9), np.sort(rng.uniform(lo, hi, 40))


def scan_all(pr, ws, E_F, ncomps, what, eig, A, lower, upper):
    """device against restatement: A = 1 and the first k components for k in ncomps, g and N; one restatement call for all"""
    ones = np.ones((1,) + A.shape[1:])
    g, N, _ = po.pairs_occ(eig, on_grid(pr, np.concatenate([A, ones])), *lower, *upper, E_F, ws)
    for states, ref in ((False, g), (True, N)):
        check(pr.ltm_occupied(ws, E_F, states=states), ref[:, -1], f"{what} A=1 {'N' if states else 'g'} nw={len(ws)}")
        for k in ncomps:
            pr.ltm_elements(A[:k])
            u = pr.ltm_occupied(ws, E_F, states=states, elements="attached")
            check(u, ref[:, :k], f"{what} ncomp={k} {'N' if states else 'g'} nw={len(ws)}")
    return g, N


# ---------------------------------------------------------------- 1. parity with the restatement
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_occupied_scans_match_the_restatement(abz, case):
    name, _, d, n, seed, npt, lower, upper, E_F, _ = case
    s = product_series(abz, case_oracle_series(case))
    src = abz.DeviceRule(s.device(), npt, None, abz._lib.WANT_EIG)
    pr = src.ltm_pairs(lower, upper)
    eig = ln.rule_eigenvalues(src)
    rng = np.random.default_rng(seed + 17)
    A = rng.standard_normal((7, src.nk, pr.nbands))  # component groups 4 + 2 + 1; 1, 2, 3 components: groups 1 | 2 | 2 + 1
    D = pr.export(x=False, w=False, eig=True)["eig"]
    coarse, fine = energy_lists(D, rng)
    ws = np.concatenate([coarse, fine])
    g, N = scan_all(pr, ws, E_F, (1, 2, 3, 7), name, eig, A, lower, upper)
    assert np.abs(g).max() > 0.0 and np.abs(N).max() > 0.0
    # the lists one by one give the same numbers as the joined list to the same bound (other windows, other chunks of work)
    pr.ltm_elements(A)
    for part, sl in ((coarse, slice(0, len(coarse))), (fine, slice(len(coarse), None))):
        check(pr.ltm_occupied(part, E_F, elements="attached"), g[sl, :7], f"{name} g, list of {len(part)}")
        check(pr.ltm_occupied(part, E_F, states=True, elements="attached"), N[sl, :7], f"{name} N, list of {len(part)}")
    pr.close()
    src.close()


def test_energy_list_longer_than_one_chunk(abz):
    """1100 energies: more than one chunk of every kernel (g 1024 / 568 / 301, N 512 / 301 / 155 for 1 / 2 / 4 components)"""
    case = CASES[1]
    name, _, d, n, seed, npt, lower, upper, E_F, _ = case
    s = product_series(abz, case_oracle_series(case))
    src = abz.DeviceRule(s.device(), npt, None, abz._lib.WANT_EIG)
    pr = src.ltm_pairs(lower, upper)
    eig = ln.rule_eigenvalues(src)
    rng = np.random.default_rng(5)
    A = rng.standard_normal((7, src.nk, pr.nbands))
    D = pr.export(x=False, w=False, eig=True)["eig"]
    ws = rng.uniform(D.min() - 0.2, D.max() + 0.2, 1100)  # (unsorted: the results come back in the caller's order)
    scan_all(pr, ws, E_F, (7,), name + " long", eig, A, lower, upper)
    pr.close()
    src.close()


@pytest.mark.parametrize("nstates", [0.5, 1.5])
def test_svo_at_its_own_fermi_level(abz, nstates):
    """SrVO3 t2g, a metal: velocity operators, 6 components, both staircase rules at the grid's own Fermi level"""
    h = svo(abz)
    src = h.device().rule(8, None, abz._lib.WANT_EIG)
    E_F, N_F = src.ltm_fermi(nstates)
    assert abs(N_F - nstates) < 1e-6
    eig = ln.rule_eigenvalues(src)
    comps = [(a, b, "re") for a in range(3) for b in range(a, 3)]
    rng = np.random.default_rng(3)
    for lower, upper in (((0, 1), (1, 2)), ((1, 1), (2, 1))):
        pr = src.ltm_pairs(lower, upper, abz.velocity_operators(h), comps)
        A = pr.ltm_elements_export()
        D = pr.export(x=False, w=False, eig=True)["eig"]
        coarse, fine = energy_lists(D, rng)
        ws = np.concatenate([coarse, fine])
        g, N, _ = po.pairs_occ(eig, on_grid(pr, A), *lower, *upper, E_F, ws)
        check(pr.ltm_occupied(ws, E_F, elements="attached"), g, f"svo {nstates} {lower}{upper} g")
        check(pr.ltm_occupied(ws, E_F, states=True, elements="attached"), N, f"svo {nstates} {lower}{upper} N")
        assert np.all(N[:, [0, 3, 5]] >= -1e-12) and N[-1, [0, 3, 5]].min() > 0.0  # sums of |M|^2 (the restatement's signed sums round)
        # the occupations remove transitions: never more than the whole-band spectrum
        whole = pr.ltm(ws, states=True, elements="attached")
        assert np.all(N[:, [0, 3, 5]] <= whole[:, [0, 3, 5]] + 1e-12)
        pr.close()


# ---------------------------------------------------------------- 2. identities that need no restatement
def gapped_series(abz, d=2, n=4, seed=31, shift=80.0):
    """a random Hermitian series whose upper two orbitals sit `shift` above the lower two: a gap between bands 1 and 2"""
    dims = (3,) * d
    c, first = rand_series(np.random.default_rng(seed), dims, n, hermitian=True)
    c = np.array(c)
    zero = tuple(-f for f in np.atleast_1d(first))  # the index of R = 0
    for a in range(n // 2, n):
        c[zero + (a, a)] += shift
    return abz.FourierSeries(c, period=1.0, first=first, ndim=d)


@pytest.mark.parametrize("d,npt", [(1, 40), (2, 7), (3, 5)])
def test_fermi_level_in_the_gap_gives_the_scans_of_the_pair_rule(abz, d, npt):
    """(i) every simplex is uncut: the closed forms see the same corners as the scan of the pair rule itself, so the two differ by the
    order of the histogram adds only: 1e-12 of the scale (at most some 1e4 terms of one sign pattern per energy, each rounded to 1.1e-16)."""
    s = gapped_series(abz, d)
    src = abz.DeviceRule(s.device(), npt, None, abz._lib.WANT_EIG)
    eig = src.export(x=False, w=False, eig=True)["eig"]
    assert eig[:, 1].max() + 10.0 < eig[:, 2].min()
    pr = src.ltm_pairs((0, 2), (2, 2))
    rng = np.random.default_rng(d)
    A = rng.standard_normal((7, src.nk, 4))
    pr.ltm_elements(A)
    D = pr.export(x=False, w=False, eig=True)["eig"]
    for ws in energy_lists(D, rng):
        for E_F in (0.5 * (eig[:, 1].max() + eig[:, 2].min()), float(eig[:, 1].max())):  # in the gap; at the top of the lower range
            for states in (False, True):
                for got, ref in ((pr.ltm_occupied(ws, E_F, states=states), pr.ltm(ws, states=states)),
                                 (pr.ltm_occupied(ws, E_F, states=states, elements="attached"), pr.ltm(ws, states=states, elements="attached"))):
                    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (d, states, E_F)
        # (ii) no occupied state, no empty state: exactly zero
        for E_F in (float(eig[:, 0].min()) - 1e-9, float(eig.min()) - 5.0, float(eig.max()), float(eig.max()) + 5.0):
            for states in (False, True):
                assert np.all(pr.ltm_occupied(ws, E_F, states=states) == 0.0)
                assert np.all(pr.ltm_occupied(ws, E_F, states=states, elements="attached") == 0.0)
    pr.close()
    src.close()


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[4]], ids=[CASES[1][0], CASES[2][0], CASES[4][0]])
def test_cumulative_jdos_above_all_transitions(abz, case):
    """(iii) N^occ(w > max Delta) = nc sum_v N_v(E_F) - nv sum_c N_c(E_F) with the per-band state counts from the source's own
    integration weights ltm_node_weights([E_F]) summed over k: the parity bound, of the number of pairs."""
    name, _, d, n, seed, npt, lower, upper, E_F, _ = case
    s = product_series(abz, case_oracle_series(case))
    src = abz.DeviceRule(s.device(), npt, None, abz._lib.WANT_EIG)
    pr = src.ltm_pairs(lower, upper)
    D = pr.export(x=False, w=False, eig=True)["eig"]
    Nb = src.ltm_node_weights(np.array([E_F]), states=True)[0].sum(axis=0)  # [n]
    ref = upper[1] * Nb[lower[0]:lower[0] + lower[1]].sum() - lower[1] * Nb[upper[0]:upper[0] + upper[1]].sum()
    got = pr.ltm_occupied([D.max() + 0.5, D.max() + 50.0], E_F, states=True)
    assert ref > 0.05
    check(got, np.array([ref, ref]), f"{name} sum rule")
    pr.close()
    src.close()


def diagonal_series(abz, d, diag):
    """H(k) = diag(f_a(k)), f_a = diag[a][0] + diag[a][1] sum_j cos 2 pi k_j"""
    n = len(diag)
    c = np.zeros((3,) * d + (n, n), dtype=np.complex128)
    for a, (c0, c1) in enumerate(diag):
        c[(1,) * d + (a, a)] = c0
        for j in range(d):
            for sgn in (0, 2):
                idx = [1] * d
                idx[j] = sgn
                c[tuple(idx) + (a, a)] += 0.5 * c1
    return abz.FourierSeries(c, period=1.0, first=(-1,) * d, ndim=d)


def test_two_exactly_degenerate_bands_give_finite_values(abz):
    """A band with itself is not a pair rule; two exactly degenerate bands (v, v + 1) are: Delta = 0 on every simplex, all of them flat.
    The DOS of a flat simplex is 0 and the count steps at w = 0 by the occupied-and-empty volume, which is empty here too: where v
    is occupied its twin is not empty."""
    s = diagonal_series(abz, 2, [(0.0, 1.0), (0.0, 1.0), (5.0, 0.5)])
    src = abz.DeviceRule(s.device(), 7, None, abz._lib.WANT_EIG)
    eig = src.export(x=False, w=False, eig=True)["eig"]
    exact = np.array_equal(eig[:, 0], eig[:, 1])
    assert np.abs(eig[:, 0] - eig[:, 1]).max() <= 1e-14
    pr = src.ltm_pairs((0, 1), (1, 1))
    ws = np.array([-0.5, 0.0, 1e-12, 0.5])
    for E_F in (0.3, float(eig[5, 0])):
        for states in (False, True):
            u = pr.ltm_occupied(ws, E_F, states=states)
            assert np.all(np.isfinite(u)), (E_F, states, u)
            if exact:  # (the solver returned the two equal diagonal entries bit for bit)
                assert np.all(u == 0.0), (E_F, states, u)
    pr.close()
    src.close()


# ---------------------------------------------------------------- 3. ties
def test_fermi_level_on_a_node_eigenvalue(abz):
    """E_F equal, bit for bit, to eigenvalues of nodes -- of the lower and of the upper range: the corner is occupied (e_v <= E_F) resp.
    not empty (e_c > E_F fails), the cut runs through the corner, and device and restatement agree under that convention."""
    case = CASES[2]
    name, _, d, n, seed, npt, lower, upper, _, _ = case
    s = product_series(abz, case_oracle_series(case))
    src = abz.DeviceRule(s.device(), npt, None, abz._lib.WANT_EIG)
    pr = src.ltm_pairs(lower, upper)
    eig = ln.rule_eigenvalues(src)
    flat = eig.reshape(-1, n)
    A = np.random.default_rng(9).standard_normal((3, src.nk, pr.nbands))
    D = pr.export(x=False, w=False, eig=True)["eig"]
    ws = np.linspace(D.min() - 0.1, D.max() + 0.1, 25)
    v_mid = np.sort(flat[:, lower[0] + 1])[len(flat) // 2]
    c_mid = np.sort(flat[:, upper[0]])[len(flat) // 2]
    for E_F in (float(v_mid), float(c_mid)):
        assert (flat == E_F).any()
        scan_all(pr, ws, E_F, (3,), f"tie at {E_F:.6f}", eig, A, lower, upper)
    pr.close()
    src.close()


def test_flat_band_at_the_fermi_level(abz):
    """An exactly flat band at E_F.  As the lower band it is occupied everywhere (e_v <= E_F): the whole-band scan.  As the upper band
    it is nowhere empty (e_c > E_F fails): exactly zero."""
    s = diagonal_series(abz, 2, [(-3.0, 1.0), (0.25, 0.0), (3.0, 1.0)])
    src = abz.DeviceRule(s.device(), 7, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(src)
    assert np.ptp(eig[..., 1]) <= 1e-14 and abs(eig[..., 1].max() - 0.25) <= 1e-14
    E_F = float(eig[..., 1].max())  # (0.25 itself when the solver returns the diagonal entry bit for bit)
    ws = np.linspace(-0.5, 7.0, 31)
    A = np.random.default_rng(4).standard_normal((2, src.nk, 1))
    up = src.ltm_pairs((1, 1), (2, 1))
    g, N = scan_all(up, ws, E_F, (2,), "flat lower band", eig, A, (1, 1), (2, 1))
    assert np.abs(g[:, -1] - up.ltm(ws)).max() <= 1e-12 * max(1.0, np.abs(g).max())
    low = src.ltm_pairs((0, 1), (1, 1))
    low.ltm_elements(A)
    for states in (False, True):
        assert np.all(low.ltm_occupied(ws, E_F, states=states) == 0.0) and np.all(low.ltm_occupied(ws, E_F, states=states, elements="attached") == 0.0)
    g0, N0, _ = po.pairs_occ(eig, None, 0, 1, 1, 1, E_F, ws)
    assert np.all(g0 == 0.0) and np.all(N0 == 0.0)
    for r in (up, low, src):
        r.close()


# ---------------------------------------------------------------- 4. sources
def test_unfolded_source(abz):
    h = svo(abz)
    cub = abz.load_bz(abz.CubicSymIBZ(), 3.85856 * np.eye(3))
    sym = abz.DeviceRule(h.device(), 8, cub.syms, abz._lib.WANT_EIG)
    unf = sym.unfold()
    E_F, _ = unf.ltm_fermi(1.0)
    pr = unf.ltm_pairs((0, 1), (1, 2))
    eig = ln.rule_eigenvalues(unf)
    D = pr.export(x=False, w=False, eig=True)["eig"]
    ws = np.linspace(D.min() - 0.01, D.max() + 0.01, 20)
    g, N, _ = po.pairs_occ(eig, None, 0, 1, 1, 2, E_F, ws)
    check(pr.ltm_occupied(ws, E_F), g[:, 0], "unfolded svo g")
    check(pr.ltm_occupied(ws, E_F, states=True), N[:, 0], "unfolded svo N")
    for r in (pr, unf, sym):
        r.close()


def test_window_of_64_pairs_of_a_40_band_source(abz):
    s = product_series(abz, orc.synthetic_wannier(40, rmax=2, seed=7))
    src = abz.DeviceRule(s.device(), 5, None, abz._lib.WANT_EIG)
    pr = src.ltm_pairs((16, 8), (24, 8))
    assert pr.nbands == 64
    eig = ln.rule_eigenvalues(src)
    E_F = float(np.median(eig[..., 16:32]))
    D = pr.export(x=False, w=False, eig=True)["eig"]
    ws = np.linspace(D.min() - 0.01, D.max() + 0.01, 12)
    g, N, census = po.pairs_occ(eig, None, 16, 8, 24, 8, E_F, ws)
    assert len(census) > 5 and N[-1, 0] > 1.0
    check(pr.ltm_occupied(ws, E_F), g[:, 0], "64 pairs g")
    check(pr.ltm_occupied(ws, E_F, states=True), N[:, 0], "64 pairs N")
    pr.close()
    src.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_launch_nothing_and_leave_the_rules_usable(abz):
    L = abz._lib
    lib = L.lib()
    n = 6
    s = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7))
    dev = s.device()
    src = abz.DeviceRule(dev, 6, None, L.WANT_EIG)
    pr = src.ltm_pairs((0, 2), (3, 3))
    A = np.random.default_rng(2).standard_normal((2, src.nk, 6))
    ws = np.linspace(0.5, 6.0, 9)
    E_F = float(np.median(src.export(x=False, w=False, eig=True)["eig"][:, 1:5]))
    good_one = pr.ltm_occupied(ws, E_F)

    def call(srch, ph, E_F=E_F, source=L.LTM_A_ONE, w=ws, nw=None, what=L.LTM_DOS, out=True):
        buf = np.full((len(ws), 2), 7.0)
        wp = None if w is None else np.ascontiguousarray(w).ctypes.data_as(L.c_f64p)
        rc = lib.abz_rule_ltm_pairs_occupied(srch, ph, float(E_F), source, wp, len(ws) if nw is None else nw, what,
                                             buf.ctypes.data_as(L.c_f64p) if out else None)
        assert np.all(buf == 7.0) or rc == 0
        return rc

    dev.ctx.prof_enable(True, kernels=[L.K_LTM, L.K_EIG])
    try:
        dev.ctx.prof_reset()

        def refused(rc, code, words=None):
            assert rc == code and len(lib.abz_last_error()) > 0, (rc, code, lib.abz_last_error())
            if words is not None:
                assert words in lib.abz_last_error(), lib.abz_last_error()
            assert dev.ctx.prof_read(L.K_LTM)[1] == 0 and dev.ctx.prof_read(L.K_EIG)[1] == 0

        h, ph = src.h, pr.h
        refused(call(h, ph, source=L.LTM_A_ELEMENTS), L.ERR_ARG, b"no elements")
        refused(call(h, ph, what=L.LTM_STATES_CORRECTED), L.ERR_UNSUPPORTED, b"curvature correction")
        refused(call(h, ph, nw=0), L.ERR_ARG)
        refused(call(h, ph, w=None), L.ERR_ARG)
        refused(call(h, ph, out=False), L.ERR_ARG)
        refused(call(h, ph, what=5), L.ERR_ARG)
        refused(call(h, ph, source=L.LTM_A_ENERGY), L.ERR_ARG)
        refused(call(h, ph, E_F=np.inf), L.ERR_ARG, b"finite")
        refused(call(h, ph, E_F=np.nan), L.ERR_ARG, b"finite")
        refused(call(ph, ph), L.ERR_UNSUPPORTED, b"pair rule")  # a pair rule as src
        refused(call(h, h), L.ERR_ARG, b"not a rule made by")    # a plain rule as pairs
    finally:
        dev.ctx.prof_enable(False)
    # rules of another grid, another series, a slab, a node list: built outside the counted stretch
    other = abz.DeviceRule(dev, 5, None, L.WANT_EIG)
    assert call(other.h, pr.h) == L.ERR_ARG and b"npt" in lib.abz_last_error()
    other.close()
    s2 = product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=8))
    foreign = abz.DeviceRule(s2.device(), 6, None, L.WANT_EIG)
    assert call(foreign.h, pr.h) == L.ERR_ARG
    foreign.close()
    s3 = product_series(abz, orc.synthetic_wannier(4, rmax=2, seed=7))  # fewer bands than the upper range needs: another series, too
    few = abz.DeviceRule(s3.device(), 6, None, L.WANT_EIG)
    assert call(few.h, pr.h) == L.ERR_ARG
    few.close()
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, 6, 2, 4, L.WANT_EIG, C.byref(slab)))
    assert call(slab, pr.h) == L.ERR_UNSUPPORTED and b"not a whole periodic grid" in lib.abz_last_error()
    assert lib.abz_rule_destroy(slab) == 0
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, 6, cub.syms, L.WANT_EIG)
    assert call(sym._h, pr.h) == L.ERR_UNSUPPORTED and b"not a whole periodic grid" in lib.abz_last_error()
    sym.close()
    honly = abz.DeviceRule(dev, 6, None, L.WANT_H)
    assert call(honly._h, pr.h) == L.ERR_ARG
    honly.close()
    # the Python layer
    with pytest.raises(ValueError, match="elements"):
        pr.ltm_occupied(ws, E_F, elements="attached")
    with pytest.raises(ValueError):
        pr.ltm_occupied(ws, E_F, elements="energy")
    with pytest.raises(ValueError, match="finite"):
        pr.ltm_occupied(ws, np.nan)
    with pytest.raises(ValueError):
        pr.ltm_occupied([], E_F)
    # both rules are as they were
    assert np.array_equal(pr.ltm_occupied(ws, E_F), good_one)
    pr.ltm_elements(A)
    assert pr.ltm_occupied(ws, E_F, elements="attached").shape == (len(ws), 2) and np.array_equal(pr.ltm_elements_export(), A)
    assert call(src.h, pr.h, source=L.LTM_A_ELEMENTS) == 0
    pr.close()
    src.close()


def test_occupied_scans_are_profiled_as_ltm(abz):
    L = abz._lib
    s = product_series(abz, case_oracle_series(CASES[3]))
    dev = s.device()
    src = abz.DeviceRule(dev, 5, None, L.WANT_EIG)
    pr = src.ltm_pairs((0, 1), (1, 2))
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        dev.ctx.prof_reset()
        pr.ltm_occupied([0.5, 1.0], CASES[3][8], states=True)
        ms, launches = dev.ctx.prof_read(L.K_LTM)
        assert launches >= 1 and ms > 0.0
    finally:
        dev.ctx.prof_enable(False)
    pr.close()
    src.close()


# ---------------------------------------------------------------- 6. the dos routes
def test_dos_routes(abz):
    L = abz._lib
    h = svo(abz)
    bz = abz.load_bz(abz.FBZ(), 3.85856 * np.eye(3))
    npt = 8
    prob = abz.DOSProblem(h, None, bz)
    src = h.device().rule(npt, None, L.WANT_EIG)
    E_F, _ = src.ltm_fermi(0.5)
    comps = [(a, b, "re") for a in range(3) for b in range(a, 3)]
    ws = np.linspace(0.02, 1.5, 16)
    rules = [src.ltm_pairs(lo, up, abz.velocity_operators(h), comps) for lo, up in (((0, 1), (1, 2)), ((1, 1), (2, 1)))]
    S = [r.ltm_occupied(ws, E_F, elements="attached") for r in rules]
    J = [r.ltm_occupied(ws, E_F) for r in rules]
    NS = [r.ltm_occupied(ws, E_F, states=True, elements="attached") for r in rules]
    assert S[0].shape == (16, 6) and np.abs(S[0]).max() > 0.0 and np.abs(J[1]).max() > 0.0
    # explicit ranges on a problem, with fermi= and with nstates=
    assert np.array_equal(abz.dos.interband(prob, ws, lower=(0, 1), upper=(1, 2), npt=npt, fermi=E_F), S[0])
    assert np.array_equal(abz.dos.interband(prob, ws, lower=(1, 1), upper=(2, 1), npt=npt, nstates=0.5), S[1])
    assert np.array_equal(abz.dos.interband(prob, ws, nocc=1, npt=npt, cumulative=True, fermi=E_F), NS[0])
    assert np.array_equal(abz.dos.joint_dos(prob, ws, nocc=1, npt=npt, fermi=E_F), J[0])
    assert np.array_equal(abz.dos.joint_dos(prob, ws, lower=(1, 1), upper=(2, 1), npt=npt, nstates=0.5), J[1])
    # all pairs v < c: the sum of the two explicit range calls
    assert np.array_equal(abz.dos.interband(prob, ws, npt=npt, nstates=0.5), S[0] + S[1])
    assert np.array_equal(abz.dos.interband(prob, ws, npt=npt, fermi=E_F, cumulative=True), NS[0] + NS[1])
    assert np.array_equal(abz.dos.joint_dos(prob, ws, npt=npt, fermi=E_F), J[0] + J[1])
    assert np.array_equal(abz.dos.joint_dos(prob, ws, npt=npt, nstates=0.5), J[0] + J[1])
    # a cache
    cache = abz.dos.init(abz.DOSProblem(h, ws, bz), abz.LTM(npt=npt, pairs=abz.BandPairs(nocc=1, operators="velocities")))
    assert np.array_equal(abz.dos.interband(cache, ws, fermi=E_F), S[0]) and np.array_equal(abz.dos.interband(cache, ws, nstates=0.5), S[0])
    assert np.array_equal(abz.dos.joint_dos(cache, ws, fermi=E_F), J[0]) and np.array_equal(abz.dos.joint_dos(cache, ws, nstates=0.5), J[0])
    assert np.array_equal(abz.dos.interband(cache, ws), rules[0].ltm(ws, elements="attached"))  # without the keywords: today's path
    sym = abz.dos.joint_dos(abz.DOSProblem(h, None, abz.load_bz(abz.CubicSymIBZ(), 3.85856 * np.eye(3))), ws, nocc=1, npt=npt, symmetric=True,
                            fermi=E_F)
    check(sym, J[0], "JDOS of the metal from irreducible nodes")
    # what does not go with occupations
    with pytest.raises(NotImplementedError, match="complex"):
        abz.dos.interband(cache, ws + 0.1j, fermi=E_F)
    with pytest.raises(NotImplementedError, match="complex"):
        abz.dos.interband(prob, ws + 0.1j, nstates=0.5, npt=npt)
    with pytest.raises(ValueError, match="correction"):
        abz.dos.interband(prob, ws, nocc=1, npt=npt, cumulative=True, correction=True, fermi=E_F)
    cor = abz.dos.init(abz.DOSProblem(h, ws, bz), abz.LTM(npt=npt, cumulative=True, correction=True, pairs=abz.BandPairs(nocc=1, operators="velocities")))
    with pytest.raises(ValueError, match="correction"):
        abz.dos.interband(cor, ws, fermi=E_F)
    with pytest.raises(ValueError, match="at most one"):
        abz.dos.joint_dos(cache, ws, fermi=E_F, nstates=0.5)
    for r in rules:
        r.close()

"""Interband spectra of metals (abz_rule_ltm_pairs_occupied), CPU side: the bindings, the new keywords of joint_dos / interband, the
argument errors of the Python layer, the numpy restatement of the device tests (tests/pairs_occ_numpy.py) against identities that
do not use it, and the census of cut cases of every input of test_gpu_ltm_pairs_occupied.py (CASES below: the seeds and Fermi
levels are picked here, on the CPU, so that every cut case is met on the device).  The kernel is checked in the GPU file."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import abz_oracle as orc
import ltm_numpy as ln
import pairs_numpy as pn
import pairs_occ_numpy as po
import wltm_numpy as wn
from test_gpu_parity import rand_series

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# The inputs of the device parity tests: (name, kind, d, bands, seed, npt, lower, upper, E_F, full).  kind "rand": rand_series on
# dims (5,) / (3, 5); "syn": orc.synthetic_wannier(n, rmax=2, seed).  `full`: every reachable pair (occupied v-corners, empty
# c-corners) occurs; otherwise (a single pair of bands, or 9 points in 1-d) each side takes all its d + 2 values.
CASES = [
    ("d1_npt9", "rand", 1, 6, 10, 9, (1, 2), (3, 3), 0.084, False),
    ("d1_npt40", "rand", 1, 6, 7, 40, (1, 2), (3, 3), 1.095, True),
    ("d2_npt7", "rand", 2, 6, 5, 7, (1, 2), (3, 3), -0.339, True),
    ("d3_npt5_n3", "syn", 3, 3, 1, 5, (0, 1), (1, 2), -0.502, True),
    ("d3_npt5_n5", "syn", 3, 5, 4, 5, (1, 2), (3, 2), 0.237, True),
    ("d3_npt12_n2", "syn", 3, 2, 1, 12, (0, 1), (1, 1), 0.236, False),
    ("d3_npt12_n3", "syn", 3, 3, 8, 12, (0, 2), (2, 1), 0.89, True),
    ("d3_npt12_n5", "syn", 3, 5, 7, 12, (0, 2), (2, 3), -0.481, True),
]
RAND_DIMS = {1: (5,), 2: (3, 5)}


def case_oracle_series(case):
    _, kind, d, n, seed = case[:5]
    if kind == "syn":
        return orc.synthetic_wannier(n, rmax=2, seed=seed)
    c, first = rand_series(np.random.default_rng(seed), RAND_DIMS[d], n, hermitian=True)
    return orc.FourierSeries(c, period=1.0, first=first, ndim=d)


def reachable(d):
    """e_c >= e_v at every corner: a corner that is not empty in c is occupied in v, so nocc + nemp >= d + 1"""
    return {(i, j) for i in range(d + 2) for j in range(d + 2) if i + j >= d + 1}


def smallest_cut_edge(eig, bands, E_F):
    """min |e_j - e_i| over the simplex edges of the bands `bands` that E_F cuts"""
    d = eig.ndim - 1
    ce = wn.corner_sets(eig[..., list(bands)], d)  # [ns, d+1, nb]
    best = math.inf
    for i in range(d + 1):
        for j in range(i + 1, d + 1):
            a, b = ce[:, i], ce[:, j]
            cut = (np.minimum(a, b) <= E_F) & (E_F < np.maximum(a, b))
            if cut.any():
                best = min(best, float(np.abs(a - b)[cut].min()))
    return best


def check_census(eig, lower, upper, E_F, full, what):
    d = eig.ndim - 1
    _, _, census = po.pairs_occ(eig, None, lower[0], lower[1], upper[0], upper[1], E_F, [1.0])
    assert census <= reachable(d), (what, census - reachable(d))
    if full:
        assert census == reachable(d), (what, reachable(d) - census)
    assert {i for i, _ in census} == set(range(d + 2)) and {j for _, j in census} == set(range(d + 2)), (what, census)
    gap = smallest_cut_edge(eig, range(lower[0], upper[0] + upper[1]), E_F)
    assert gap >= 1e-6, (what, gap)  # no cut edge is so short that the parity bound would have to widen


# ---------------------------------------------------------------- 1. bindings
def test_ltm_pairs_occupied_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert re.search(r"^int abz_rule_ltm_pairs_occupied\(abz_rule\* src, abz_rule\* pairs, double E_F, int source, const double\* w, int nw, "
                     r"int what,\s*double\* out(?: /\*.*?\*/)?\);", hdr, flags=re.M)
    name = "abz_rule_ltm_pairs_occupied"
    assert name in L.PROTOTYPES and hasattr(L.lib(), name) and ":" + name in jl and "function ltm_pairs_occupied(" in jl
    assert len(L.PROTOTYPES[name][1]) == 8
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_LTM_A_ONE"] == 2 == L.LTM_A_ONE and defs["ABZ_LTM_A_ELEMENTS"] == 0 and defs["ABZ_LTM_A_ENERGY"] == 1
    assert defs["ABZ_VERSION"] == 502 and defs["ABZ_K_COUNT"] == 8
    assert hdr.index("int abz_rule_ltm_pairs(") < hdr.index("Interband spectra of a metal") < hdr.index("int abz_rule_ltm_pairs_occupied(")
    doc = hdr[hdr.index("Pair rules: joint density of states"):hdr.index("int abz_rule_ltm_pairs(")]
    assert "partial occupations" in doc and "abz_rule_ltm_pairs_occupied" in doc
    assert list(inspect.signature(abz.series.PairRule.ltm_occupied).parameters) == ["self", "ws", "fermi", "states", "elements"]


def test_new_keywords_come_last_and_old_signatures_stand():
    import autobzcore.jl_amd as abz
    j = inspect.signature(abz.dos.joint_dos).parameters
    assert list(j) == ["prob_or_cache", "ws", "nocc", "lower", "upper", "npt", "cumulative", "symmetric", "fermi", "nstates"]
    i = inspect.signature(abz.dos.interband).parameters
    assert list(i) == ["prob_or_cache", "ws_or_zs", "nocc", "lower", "upper", "operators", "components", "basis", "npt", "cumulative",
                       "correction", "fermi", "nstates"]
    for p in (j, i):
        assert p["fermi"].default is None and p["nstates"].default is None and p["npt"].default == 50 and p["cumulative"].default is False
    assert i["operators"].default == "velocities" and j["symmetric"].default is False


def test_python_argument_errors_come_before_the_device():
    import autobzcore.jl_amd as abz
    c, first = rand_series(np.random.default_rng(3), (3, 3, 3), 4, hermitian=True)
    s = abz.FourierSeries(c, period=1.0, first=first, ndim=3)
    prob = abz.DOSProblem(s, None, abz.load_bz(abz.FBZ(), np.eye(3)))
    for f in (abz.dos.joint_dos, abz.dos.interband):
        with pytest.raises(ValueError, match="at most one"):
            f(prob, [1.0], nocc=2, npt=4, fermi=0.0, nstates=2.0)
    with pytest.raises(NotImplementedError, match="complex"):
        abz.dos.interband(prob, [1.0 + 0.1j], nocc=2, npt=4, fermi=0.0)
    with pytest.raises(NotImplementedError, match="complex"):
        abz.dos.interband(prob, [1.0 + 0.1j], npt=4, nstates=1.5)
    with pytest.raises(ValueError, match="correction"):
        abz.dos.interband(prob, [1.0], nocc=2, npt=4, cumulative=True, correction=True, fermi=0.0)
    with pytest.raises(ValueError, match="operators"):
        abz.dos.interband(prob, [1.0], operators=None, npt=4, fermi=0.0)


# ---------------------------------------------------------------- 2. the restatement against identities that do not use it
IDENT = [CASES[1], CASES[2], CASES[3]]


def ident_input(case, ncomp=3):
    name, _, d, n, seed, npt, lower, upper, E_F, _ = case
    eig = ln.grid_eigenvalues(case_oracle_series(case), min(npt, 12))
    A = np.random.default_rng(seed + 50).standard_normal((ncomp,) + eig.shape[:d] + (lower[1] * upper[1],))
    return eig, A, lower, upper, E_F


def pair_grid(eig, lower, upper):
    d = eig.ndim - 1
    D = pn.pair_energies(eig.reshape(-1, eig.shape[-1]), lower[0], lower[1], upper[0], upper[1])
    return D.reshape(eig.shape[:d] + (D.shape[-1],))


@pytest.mark.parametrize("case", IDENT, ids=[c[0] for c in IDENT])
def test_fermi_level_in_a_gap_gives_the_whole_band_scans(case):
    """(i) every simplex is uncut: the restatement is wltm on the pair energies, to 1e-12 of the scale (the same terms in another order)."""
    eig, A, lower, upper, _ = ident_input(case)
    eig = eig.copy()
    shift = eig[..., :upper[0]].max() - eig[..., upper[0]:].min() + 0.5
    eig[..., upper[0]:] += shift  # (stays ascending) a gap of 0.5 between the ranges
    E_F = eig[..., :upper[0]].max() + 0.25
    D = pair_grid(eig, lower, upper)
    ws = np.linspace(D.min() - 0.1, D.max() + 0.1, 17)
    g, N, census = po.pairs_occ(eig, A, *lower, *upper, E_F, ws)
    gr, Nr = wn.wltm(D, A, ws)
    d = eig.ndim - 1
    assert census == {(d + 1, d + 1)}
    for got, ref in ((g, gr), (N, Nr)):
        assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    # and at the upper edge of the lower range itself: a corner with e_v == E_F is occupied
    g2, N2, _ = po.pairs_occ(eig, A, *lower, *upper, eig[..., :upper[0]].max(), ws)
    assert np.abs(g2 - gr).max() <= 1e-12 * max(1.0, np.abs(gr).max()) and np.abs(N2 - Nr).max() <= 1e-12 * max(1.0, np.abs(Nr).max())


@pytest.mark.parametrize("case", IDENT, ids=[c[0] for c in IDENT])
def test_no_occupied_or_no_empty_state_gives_exactly_zero(case):
    """(ii) E_F below every e_v, or at or above every e_c"""
    eig, A, lower, upper, _ = ident_input(case)
    D = pair_grid(eig, lower, upper)
    ws = np.linspace(D.min() - 0.1, D.max() + 0.1, 9)
    ev = eig[..., lower[0]:lower[0] + lower[1]]
    ec = eig[..., upper[0]:upper[0] + upper[1]]
    for E_F in (ev.min() - 1e-9, ev.min() - 3.0, ec.max(), ec.max() + 2.0):
        g, N, _ = po.pairs_occ(eig, A, *lower, *upper, E_F, ws)
        assert np.all(g == 0.0) and np.all(N == 0.0), E_F


@pytest.mark.parametrize("case", CASES[:5], ids=[c[0] for c in CASES[:5]])
def test_cumulative_jdos_above_all_transitions_counts_occupied_minus_doubly_occupied(case):
    """(iii) N^occ(w > max Delta) = nc sum_v N_v(E_F) - nv sum_c N_c(E_F), per-band state counts from ltm_numpy"""
    eig, _, lower, upper, E_F = ident_input(case)
    D = pair_grid(eig, lower, upper)
    _, N, _ = po.pairs_occ(eig, None, *lower, *upper, E_F, [D.max() + 0.5])
    Nb = [ln.ltm(eig[..., b:b + 1], [E_F])[1][0] for b in range(eig.shape[-1])]
    ref = upper[1] * sum(Nb[lower[0]:lower[0] + lower[1]]) - lower[1] * sum(Nb[upper[0]:upper[0] + upper[1]])
    assert ref > 0.05 and abs(N[0, 0] - ref) <= 1e-12 * max(1.0, lower[1] * upper[1])


def test_one_dimensional_two_band_model_by_hand():
    """e_v = -1 + k, e_c = 1 + 3 k on one segment k in [0, 1] of a 2-point grid (and back): with E_F = -0.5 the occupied part is
    k < 1/2, Delta = 2 + 2 k there, so J^occ = 1/2 on 2 <= w < 3 (each of the two segments has weight 1/2) and N^occ(w) = (w - 2) / 2."""
    eig = np.array([[-1.0, 1.0], [0.0, 4.0]])
    g, N, census = po.pairs_occ(eig, None, 0, 1, 1, 1, -0.5, [2.5, 2.999, 3.5])
    assert census == {(1, 2)}
    assert np.allclose(g[:, 0], [0.5, 0.5, 0.0], rtol=0, atol=1e-14) and np.allclose(N[:, 0], [0.25, 0.4995, 0.5], rtol=0, atol=1e-14)


# ---------------------------------------------------------------- 3. the census of the device inputs
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_census_of_the_device_inputs_covers_every_cut_case(case):
    name, _, d, n, seed, npt, lower, upper, E_F, full = case
    eig = ln.grid_eigenvalues(case_oracle_series(case), npt)
    assert eig.shape == (npt,) * d + (n,)
    check_census(eig, lower, upper, E_F, full, name)


def svo_fermi(eig, nstates):
    """The Fermi level of ltm_numpy's state count by bisection (the device's ltm_fermi agrees to its tol)"""
    lo, hi = eig.min(), eig.max()
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if ln.ltm(eig, [mid])[1][0] >= nstates:
            hi = mid
        else:
            lo = mid
    return hi


@pytest.mark.parametrize("nstates", [0.5, 1.5])
def test_census_of_the_svo_input(nstates):
    """SrVO3 t2g on 8^3 at the grid's own Fermi level of 0.5 and 1.5 states, all pairs v < c as the two staircase rules together"""
    import autobzcore.jl_amd as abz
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    eig = ln.grid_eigenvalues(orc.FourierSeries(s.c, period=1.0, first=s.first, ndim=3), 8)
    E_F = svo_fermi(eig, nstates)
    census = set()
    for lower, upper in (((0, 1), (1, 2)), ((1, 1), (2, 1))):
        census |= po.pairs_occ(eig, None, *lower, *upper, E_F, [1.0])[2]
    assert census <= reachable(3)
    assert {i for i, _ in census} == set(range(5)) and {j for _, j in census} == set(range(5)), census
    assert smallest_cut_edge(eig, range(3), E_F) >= 1e-6

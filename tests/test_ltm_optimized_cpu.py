"""Optimized tetrahedron method (Kawamura, Gohda, Tsuneyuki, PRB 89, 094515), CPU side: the projection P derived from its
definition in exact rationals (tests/optltm_numpy.py), the restatement's sums against the geometric restatement of
wltm_numpy.py, what the rule is for -- N(E) at a fixed energy --, the bindings of abz_rule_ltm_optimized and the argument checks
of the Python front end.  The device kernel is checked against the same restatement in test_gpu_ltm_optimized.py."""
import inspect
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import optltm_numpy as on
import wltm_numpy as wn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 1260 P as the issue and the published table give it; the code under test holds its own copy (kernels_ltm_opt.hip)
TABLE = [
    [1440, 0, 30, 0, -38, 7, 17, -28, -56, 9, -46, 9, -38, -28, 17, 7, -18, -18, 12, -18],
    [0, 1440, 0, 30, -28, -38, 7, 17, 9, -56, 9, -46, 7, -38, -28, 17, -18, -18, -18, 12],
    [30, 0, 1440, 0, 17, -28, -38, 7, -46, 9, -56, 9, 17, 7, -38, -28, 12, -18, -18, -18],
    [0, 30, 0, 1440, 7, 17, -28, -38, 9, -46, 9, -56, -28, 17, 7, -38, -18, 12, -18, -18],
]


@pytest.fixture(scope="module")
def P():
    return on.projection()


# ---------------------------------------------------------------- 1. the projection, from its definition
def test_projection_is_the_published_table(P):
    assert len(P) == 4 and all(len(row) == 20 for row in P)
    scaled = [[x * 1260 for x in row] for row in P]
    assert all(x.denominator == 1 for row in scaled for x in row)
    assert [[int(x) for x in row] for row in scaled] == TABLE


def test_projection_rows_sum_to_one(P):
    assert [sum(row) for row in P] == [Fraction(1)] * 4
    assert [sum(abs(x) for x in row) for row in P] == [Fraction(1836, 1260)] * 4


def test_stencil_lies_in_the_4_cube():
    for perm in itertools.permutations(range(3)):
        p = on.points(perm)
        assert p.shape == (20, 3) and p.min() == -1 and p.max() == 2
        assert len({tuple(q) for q in p}) == 20
        # corner 0, e_a, e_a + e_b, (1, 1, 1)
        assert p[0].tolist() == [0, 0, 0] and p[3].tolist() == [1, 1, 1] and p[1].sum() == 1 and p[2].sum() == 2


def test_projection_reproduces_affine_functions(P):
    """the 20 values of an affine function -> its 4 corner values, exactly, on every path"""
    coef = [Fraction(3, 7), Fraction(-5, 3), Fraction(2, 9), Fraction(11, 13)]
    for perm in itertools.permutations(range(3)):
        pts = on.points(perm)
        f = [coef[0] + sum(coef[1 + ax] * int(q[ax]) for ax in range(3)) for q in pts]
        for m in range(4):
            assert sum(P[m][j] * f[j] for j in range(20)) == f[m]


def test_residual_of_a_random_cubic_is_orthogonal_to_linear_functions(P):
    """int (cubic - linear fit) * {1, u, v, w} over the simplex = 0, in exact rationals, for a random cubic given by its 20 values"""
    rng = np.random.default_rng(3)
    vals = [Fraction(int(v), 97) for v in rng.integers(-500, 500, 20)]
    C = on.cubic_coefficients()
    cub = [sum(C[q][j] * vals[j] for j in range(20)) for q in range(20)]  # coefficients of the monomials
    # the cubic interpolates the 20 values
    for (u, v, w), f in zip(on.barycentric(), vals):
        assert sum(c * u ** i * v ** j * w ** k for c, (i, j, k) in zip(cub, on.MONOMIALS)) == f
    corner = [sum(P[m][j] * vals[j] for j in range(20)) for m in range(4)]
    # the linear fit sum_m x'_m lambda_m as coefficients of (1, u, v, w)
    lin = [sum(corner[m] * on.LAMBDA[m][t] for m in range(4)) for t in range(4)]
    unit = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
    for (du, dv, dw) in unit:
        cubic_part = sum(c * on.moment(i + du, j + dv, k + dw) for c, (i, j, k) in zip(cub, on.MONOMIALS))
        linear_part = sum(l * on.moment(a + du, b + dv, c + dw) for l, (a, b, c) in zip(lin, unit))
        assert cubic_part == linear_part
    assert any(corner[m] != vals[m] for m in range(4))  # the fit moved the corners


# ---------------------------------------------------------------- 2. the restatement's sums
def random_grid(npt, n, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.standard_normal((npt, npt, npt, n)), axis=-1)


def test_sums_on_plain_corners_are_the_geometric_restatement():
    """optimized=False feeds the closed-form corner weights the 4 corner values themselves: wltm_numpy.py's sub-simplex volumes
    and cut areas give the same g_A and N_A."""
    eig = random_grid(5, 2, 7)
    A = np.random.default_rng(8).standard_normal((3,) + eig.shape)
    Es = np.concatenate([[eig.min() - 1.0], np.linspace(eig.min(), eig.max(), 9)[1:-1] + 0.0123, [eig.max() + 1.0]])
    g_ref, N_ref = wn.wltm(eig, A, Es)
    g = on.optltm(eig, A, Es, False, optimized=False)
    N = on.optltm(eig, A, Es, True, optimized=False)
    scale = max(1.0, np.abs(N_ref).max(), np.abs(g_ref).max())
    print(f"closed forms against the geometric restatement: g {np.abs(g - g_ref).max():.2e}, N {np.abs(N - N_ref).max():.2e}")
    assert np.abs(g - g_ref).max() <= 1e-11 * scale and np.abs(N - N_ref).max() <= 1e-11 * scale
    ge, Ne = wn.wltm(eig, eig, Es)
    assert np.abs(on.optltm(eig, "energy", Es, True, optimized=False) - Ne).max() <= 1e-11 * scale


def test_optimized_sums_identities():
    eig = random_grid(4, 2, 11)
    lo, hi = eig.min(), eig.max()
    w = hi - lo
    # e' stays within (1836 / 1260 - 1) / 2 of the width outside the eigenvalues
    Es = np.array([lo - 0.25 * w, hi + 0.25 * w])
    N = on.optltm(eig, None, Es, True)
    assert N[0, 0] == 0.0 and abs(N[1, 0] - 2.0) <= 1e-13
    assert np.all(on.optltm(eig, None, Es, False) == 0.0)
    ones = np.ones((1,) + eig.shape)
    mid = np.linspace(lo, hi, 7)
    assert np.abs(on.optltm(eig, ones, mid, True) - on.optltm(eig, None, mid, True)).max() <= 1e-13
    # the optimized rule is another rule
    assert np.abs(on.optltm(eig, None, mid, True) - on.optltm(eig, None, mid, True, optimized=False)).max() > 1e-3


# ---------------------------------------------------------------- 2b. the cases of the device test
# Random Hermitian series of 3 x 3 x 3 coefficients, (bands, seed): nothing relates their three axes, so a transposed or mirrored
# stencil shows.  A near-flat simplex amplifies the rounding of e' in the closed forms; these seeds are the ones for which the
# restatement in f64 and in longdouble agrees to 1e-10 of the scale at every grid and energy list of the device test (checked below),
# so that the device's 1e-9 is a statement about the kernel.
SEEDS = {1: 101, 3: 303}
GRIDS = (3, 5, 7, 8)   # the stencil wraps onto itself | 125 cells, less than one block | a ragged second block, odd | even


def case_coefficients(n):
    rng = np.random.default_rng(SEEDS[n])
    c = rng.standard_normal((3, 3, 3, n, n)) + 1j * rng.standard_normal((3, 3, 3, n, n))
    return 0.5 * (c + np.conj(np.swapaxes(c[::-1, ::-1, ::-1], -1, -2))), (-1, -1, -1)


def case_elements(n, npt):
    """[5, npt^3, n]: 1, 3 and 5 components are the group tails 1 | 2 + 1 | 4 + 1"""
    return np.random.default_rng(1000 * n + npt).standard_normal((5, npt ** 3, n))


def energy_lists(eig):
    """five irregular energies, one below and one above every e' (which leave the eigenvalues' range by less than 0.23 of its
    width), and an equispaced list of 64 (the arithmetic first index of the window)"""
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    return {"irregular": np.array([lo - 0.3 * w, lo + 0.137 * w, lo + 0.52 * w, lo + 0.861 * w, hi + 0.3 * w]),
            "equispaced": np.linspace(lo - 0.05 * w, hi + 0.05 * w, 64)}


def sources(eig, A):
    """label -> the restatement's `A` argument"""
    grid = A.reshape((A.shape[0],) + eig.shape)
    return {"one": None, "energy": "energy", "elements": grid}


@pytest.mark.parametrize("n", sorted(SEEDS))
@pytest.mark.parametrize("npt", GRIDS)
def test_cases_are_well_conditioned(n, npt):
    import abz_oracle as orc
    import ltm_numpy as ln
    c, first = case_coefficients(n)
    eig = ln.grid_eigenvalues(orc.FourierSeries(c, period=1.0, first=first, ndim=3), npt)
    A = case_elements(n, npt)
    worst = 0.0
    for label, Es in energy_lists(eig).items():
        for src, arg in sources(eig, A).items():
            for states in (False, True):
                u = on.optltm(eig, arg, Es, states)
                v = on.optltm(eig, arg, Es, states, dtype=np.longdouble)
                worst = max(worst, float(np.abs(u - v).max()) / max(1.0, float(np.abs(v).max())))
    print(f"n = {n}, npt = {npt}: f64 against longdouble {worst:.2e} of the scale")
    assert worst <= 1e-10


# ---------------------------------------------------------------- 3. what the rule is for
def test_state_count_at_a_fixed_energy_converges_faster():
    """N(-1.3) of e(k) = -2 sum_i cos 2 pi k_i + 0.5 cos 2 pi (k_1 + k_2), errors against the optimized sum at npt = 64, the finest
    grid this test affords (the optimized error there is below 3e-7 by the order seen from 8 to 32, against 8.9e-5 at 16).
    Condition: the optimized error at npt = 16 is at most a fifth of the plain error at npt = 16.  Measured here against
    npt = 64: plain -2.758e-03, optimized -8.978e-05, ratio 30.7 (against npt = 96 the ratio was 31)."""
    E = [-1.3]
    ref = on.optltm(on.issue_band(64), None, E, True)[0, 0]
    eig = on.issue_band(16)
    plain = on.optltm(eig, None, E, True, optimized=False)[0, 0] - ref
    opt = on.optltm(eig, None, E, True)[0, 0] - ref
    print(f"N(-1.3) at npt = 16 against the optimized sum at 64: plain {plain:+.3e}, optimized {opt:+.3e}, ratio {abs(plain) / abs(opt):.1f}")
    assert abs(opt) <= abs(plain) / 5.0


# ---------------------------------------------------------------- 4. bindings
def test_optimized_bindings():
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    assert re.search(r"^int abz_rule_ltm_optimized\(abz_rule\* r, int source, const double\* E, int nE, int what, double\* out\);", hdr,
                     flags=re.M)
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_VERSION"] == 502 and defs["ABZ_K_COUNT"] == 8
    assert (defs["ABZ_LTM_A_ELEMENTS"], defs["ABZ_LTM_A_ENERGY"], defs["ABZ_LTM_A_ONE"]) == (L.LTM_A_ELEMENTS, L.LTM_A_ENERGY, L.LTM_A_ONE)
    assert L.PROTOTYPES["abz_rule_ltm_optimized"] == L.PROTOTYPES["abz_rule_ltm_weighted"]
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert ":abz_rule_ltm_optimized" in jl and "function ltm_optimized(" in jl
    mk = open(os.path.join(ROOT, "autobzcore.jl_amd", "csrc", "Makefile")).read()
    assert "kernels_ltm_opt.o" in mk
    # a null handle is refused before anything else is looked at
    assert L.lib().abz_rule_ltm_optimized(None, L.LTM_A_ONE, None, 1, L.LTM_DOS, None) == L.ERR_ARG
    assert b"null rule handle" in L.lib().abz_last_error()


# ---------------------------------------------------------------- 5. the Python front end
def test_optimized_front_end_arguments():
    import autobzcore.jl_amd as abz
    assert abz.LTM().optimized is False
    alg = abz.LTM(optimized=True, cumulative=True, elements="energy")
    assert alg.optimized is True and alg.cumulative and alg.correction is False
    assert abz.LTM(optimized=True, elements="orbitals", eigenvectors="device").optimized
    assert abz.LTM(optimized=True, elements=lambda x, eig: eig[None]).optimized
    assert abz.LTM(optimized=True, elements=abz.dos.BandExpectation([None])).optimized
    assert abz.LTM(optimized=True, symmetric=True).symmetric
    with pytest.raises(ValueError, match="correction"):
        abz.LTM(optimized=True, cumulative=True, elements="energy", correction=True)
    with pytest.raises(ValueError, match="eta"):
        abz.LTM(optimized=True, eta=0.1)
    with pytest.raises(ValueError, match="pairs"):
        abz.LTM(optimized=True, pairs=abz.dos.BandPairs(nocc=1))
    assert list(inspect.signature(abz.DeviceRule.ltm_optimized).parameters) == ["self", "Es", "states", "elements"]
    assert list(inspect.signature(abz.DeviceRule.ltm_fermi_optimized).parameters) == ["self", "nstates", "tol"]
    f = inspect.signature(abz.dos.fermi_level).parameters
    assert list(f) == ["prob_or_cache", "nstates", "tol", "optimized"] and f["optimized"].default is None


def test_optimized_is_refused_below_three_dimensions_and_on_shards():
    """the refusals the front end makes itself, before a device is asked for anything"""
    import autobzcore.jl_amd as abz
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    bz = abz.load_bz(abz.FBZ(), [[2 * np.pi]])
    with pytest.raises(NotImplementedError, match="d = 3"):
        abz.dos.init(abz.DOSProblem(h, 0.3, bz), abz.LTM(optimized=True))

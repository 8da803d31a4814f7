"""Tetrahedron Green's function with matrix elements, CPU side: the numpy restatement (tests/gwltm_numpy.py) against the pure
recursion in mpmath (60 correct digits: gwltm_numpy.MP_DPS says how many it carries for that), a Monte-Carlo mean, its own identities and limits, and the bindings of abz_rule_ltm_green_weighted.  The device kernel
is checked against the same restatement in test_gpu_ltm_green_weighted.py."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import abz_oracle as orc
import gltm_numpy as gn
import gwltm_numpy as gw
import ltm_numpy as ln
import wltm_numpy as wn
from test_ltm_green_cpu import FIVE, MP_CASES, MP_ETAS, mp_energies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0**-52

# ---------------------------------------------------------------- 1. the corner weights against mpmath
# The worst error of a corner weight, max_i |W_i - W_i,mp| / max_i |W_i,mp| per distinct simplex, over all of MP_CASES x MP_ETAS x
# mp_energies, in units of eps = 2^-52, as printed by `PYTHONPATH=oracle python tests/test_ltm_green_weighted_cpu.py`
# (int3_8 233.9, int2_16 63.5, graphene_12 59.1, syn4_5 300.6; the reference at gwltm_numpy.MP_DPS digits).
WORST_WEIGHT_EPS = 300.6
assert WORST_WEIGHT_EPS <= 1e3  # the cap of the trace's test: a larger value means the evaluation rule is wrong

# The worst deviations from the two identities over the same set, against the restatement's own J, in units of eps:
# |sum_i W_i - J| / |J| and |sum_i x_i W_i - (z J - 1)| / (|z J| + 1) (sum: int3_8 32.3, int2_16 21.7, graphene_12 12.8,
# syn4_5 46.0; first moment: 35.1, 10.0, 8.5, 64.0).
WORST_SUM_EPS = 46.0
WORST_MOMENT_EPS = 64.0


def case_simplices(name):
    make, npt = MP_CASES[name]
    eig = ln.grid_eigenvalues(make(), npt)
    return eig, np.unique(ln.kuhn_simplices(eig), axis=0)


def mp_worst(name):
    eig, e = case_simplices(name)
    worst, where = 0.0, None
    for eta in MP_ETAS:
        for E in mp_energies(eig):
            w, row = gw.worst_weight_error(e, complex(E, eta))
            if w > worst:
                worst, where = w, (row, complex(E, eta))
    return worst, where


def identity_worst(name):
    """(worst |sum W - J| / |J|, worst |sum x W - (z J - 1)| / (|z J| + 1)) in eps over the case's simplices and values of z."""
    eig, e = case_simplices(name)
    s0 = s1 = 0.0
    for eta in MP_ETAS:
        for E in mp_energies(eig):
            z = complex(E, eta)
            W = gw.simplex_weights(e, z)
            J = gn.simplex_J(e, z)
            s0 = max(s0, float((np.abs(W.sum(axis=1) - J) / np.abs(J)).max()))
            s1 = max(s1, float((np.abs((e * W).sum(axis=1) - (z * J - 1.0)) / (np.abs(z * J) + 1.0)).max()))
    return s0 / EPS, s1 / EPS


@pytest.mark.parametrize("name", list(MP_CASES))
def test_weights_vs_mpmath(name):
    """Every corner weight of every distinct simplex against the pure recursion in mpmath (gwltm_numpy.MP_DPS digits, of which the
    cancellation between corners an ulp apart leaves 60); bound 4 x the worst measured, the trace test's margin: the restatement's
    error is deterministic, the factor covers other libm builds."""
    worst, where = mp_worst(name)
    print(f"corner weights vs mpmath {name}: worst error {worst:.1f} eps of max|W| (bound {4 * WORST_WEIGHT_EPS:.0f}) at {where}")
    assert worst <= 4 * WORST_WEIGHT_EPS, (name, worst, where)


@pytest.mark.parametrize("name", list(MP_CASES))
def test_weight_identities(name):
    """sum_i W_i = J and sum_i x_i W_i = z J - 1 per simplex, against the restatement's own J; bound 4 x the worst measured."""
    s0, s1 = identity_worst(name)
    print(f"corner weight identities {name}: sum {s0:.1f} eps (bound {4 * WORST_SUM_EPS:.0f}), first moment {s1:.1f} eps "
          f"(bound {4 * WORST_MOMENT_EPS:.0f})")
    assert s0 <= 4 * WORST_SUM_EPS and s1 <= 4 * WORST_MOMENT_EPS, (name, s0, s1)


# ---------------------------------------------------------------- 2. Monte-Carlo check of the weights
@pytest.mark.parametrize("m", [2, 3])
def test_W_is_the_mean_over_the_simplex(m):
    """W_i against the mean of lambda_i / (z - e) over 4e5 uniform points of a random triangle / tetrahedron, z = 0.3 + 0.2i;
    statistical error about 2e-3, bound 1e-2 relative to max |W|."""
    rng = np.random.default_rng(4321 + m)
    x = np.sort(rng.uniform(-1.0, 1.0, m + 1))
    z = 0.3 + 0.2j
    lam = rng.dirichlet(np.ones(m + 1), size=400_000)
    mc = (lam / (z - lam @ x)[:, None]).mean(axis=0)
    W = gw.simplex_weights(x, z)[0]
    rel = np.abs(W - mc).max() / np.abs(mc).max()
    print(f"W vs Monte Carlo m={m}: relative deviation {rel:.2e}")
    assert rel <= 1e-2


# ---------------------------------------------------------------- 3. equal and nearly equal corners
def test_equal_and_nearly_equal_corners():
    z = 0.25 + 1e-8j
    for m in (1, 2, 3):
        for zz in (z, 0.3 + 0.2j, 1e8j, -4.0 + 1e-8j):
            W = gw.simplex_weights(np.full(m + 1, 0.25), zz)[0]
            assert np.all(W == (1.0 / (np.array([zz]) - 0.25))[0] / (m + 1))  # 1 / ((m + 1) u), numpy's own reciprocal
        # two equal corners: the same multiset, the same bits
        if m >= 2:
            x = np.array([0.1, 0.6, 0.6, 0.9][:m + 1])
            for zz in (z, 0.3 + 0.2j, 0.6 + 1e-4j):
                W = gw.simplex_weights(x, zz)[0]
                assert W[1] == W[2] and np.all(np.isfinite(W.view(np.float64)))
        # one ulp apart: finite, and close to 1 / ((m + 1) u)
        x = np.array([0.25] * m + [np.nextafter(0.25, 1.0)])
        W = gw.simplex_weights(x, z)[0]
        assert np.all(np.isfinite(W.view(np.float64)))
        assert np.abs(W - 1.0 / ((m + 1) * (z - 0.25))).max() <= 1e-7 * np.abs(W).max()
    x = [0.1, 0.2, 0.5, 0.9]
    assert np.array_equal(gw.simplex_weights_any(x, 0.3 - 0.2j), np.conj(gw.simplex_weights(x, 0.3 + 0.2j)))
    eig = ln.grid_eigenvalues(orc.tb_integer(2), 6)
    zs = np.array([0.4 + 1e-2j, -1.3 + 0.5j])
    assert np.array_equal(gw.green_weighted(eig, eig, np.conj(zs)), np.conj(gw.green_weighted(eig, eig, zs)))


def test_restatement_identities_on_a_grid():
    """On a whole grid: A = 1 gives the trace, A = e gives z tr G - n (to rounding), and the components do not mix."""
    eig = ln.grid_eigenvalues(orc.synthetic_wannier(4, rmax=1, seed=3), 5)
    n = eig.shape[-1]
    zs = np.array([0.2 + 1e-2j, -0.5 + 0.3j, 0.1 - 1e-4j])
    rng = np.random.default_rng(5)
    A = np.stack([np.ones_like(eig), eig, rng.standard_normal(eig.shape)])
    G = gw.green_weighted(eig, A, zs)
    t = gn.green_trace(eig, zs)
    scale = max(1.0, np.abs(t).max())
    assert np.abs(G[:, 0] - t).max() <= 1e-12 * scale
    assert np.abs(G[:, 1] - (zs * t - n)).max() <= 1e-12 * scale * max(1.0, np.abs(zs).max())
    assert np.abs(G[:, 2] - gw.green_weighted(eig, A[2], zs)[:, 0]).max() <= 1e-13 * max(1.0, np.abs(G[:, 2]).max())


# ---------------------------------------------------------------- 4. eta -> 0
def test_limit_to_eta_zero():
    """-Im G_A(E + i eta) / pi with A = e tends to g_A(E) of wltm_numpy linearly in eta: on tb_integer(3) at npt = 48 the
    difference at 1e-5 is at most 0.02 x that at 1e-3."""
    eig = ln.grid_eigenvalues(orc.tb_integer(3), 48)
    g, _ = wn.wltm(eig, eig, FIVE)
    etas = (1e-3, 1e-5)
    u = -gw.green_weighted(eig, eig, [complex(E, eta) for eta in etas for E in FIVE]).imag / math.pi  # (one pass over the grid)
    d = {eta: np.abs(u[i * len(FIVE):(i + 1) * len(FIVE)] - g).max() for i, eta in enumerate(etas)}
    print(f"|broadened g_A - g_A|: {d[1e-3]:.2e} at eta=1e-3, {d[1e-5]:.2e} at eta=1e-5, ratio {d[1e-5] / d[1e-3]:.4f}")
    assert d[1e-5] <= 0.02 * d[1e-3]


# ---------------------------------------------------------------- 5. bindings
def test_ltm_green_weighted_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    assert "abz_rule_ltm_green_weighted" in L.PROTOTYPES
    assert re.search(r"^int abz_rule_ltm_green_weighted\(abz_rule\* r, int source, const double\* z(?: /\*.*?\*/)?, int nz, "
                     r"double\* out(?: /\*.*?\*/)?\);", hdr, flags=re.M)
    assert hasattr(L.lib(), "abz_rule_ltm_green_weighted")
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert ":abz_rule_ltm_green_weighted" in jl
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_K_COUNT"] == 8 and defs["ABZ_VERSION"] == 502
    assert hasattr(abz.dos, "green_weighted")
    assert "elements" in inspect.signature(abz.DeviceRule.ltm_green).parameters


def test_ltm_eta_elements_arguments():
    import autobzcore.jl_amd as abz
    a = abz.LTM(eta=0.1, elements="energy")
    assert a.eta == 0.1 and a.elements == "energy"
    b = abz.LTM(npt=8, eta=1e-2, elements="orbitals", eigenvectors="device", orbitals=[2, 0])
    assert b.elements == "orbitals" and b.eigenvectors == "device" and b.orbitals == (2, 0)
    assert callable(abz.LTM(eta=0.1, elements=lambda x, e: e).elements)
    assert abz.LTM(eta=0.1, elements="energy", symmetric=True).symmetric is True
    for kw in ({"elements": np.ones((8, 1))}, {"elements": "energy", "cumulative": True}, {"elements": "bands"},
               {"elements": "energy", "cumulative": True, "correction": True}, {"elements": "energy", "correction": True},
               {"elements": "energy", "eigenvectors": "device"}, {"elements": "orbitals", "orbitals": [0]}):
        with pytest.raises(ValueError):
            abz.LTM(eta=0.1, **kw)


def test_ltm_eta_elements_fails_loudly_without_gpu():
    import torch
    import autobzcore.jl_amd as abz
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    bz = abz.load_bz(abz.FBZ(), [[2 * np.pi]])
    with pytest.raises(abz.AbzError):
        abz.dos.init(abz.DOSProblem(h, 0.0, bz), abz.LTM(eta=0.1, elements="energy"))


if __name__ == "__main__":  # prints the constants above:  PYTHONPATH=oracle python tests/test_ltm_green_weighted_cpu.py
    per = {name: mp_worst(name) for name in MP_CASES}
    for name, (w, where) in per.items():
        print(f"{name}: worst corner weight error {w:.1f} eps at {where}")
    print(f"WORST_WEIGHT_EPS = {max(w for w, _ in per.values()):.1f}")
    ids = {name: identity_worst(name) for name in MP_CASES}
    for name, (s0, s1) in ids.items():
        print(f"{name}: sum {s0:.1f} eps, first moment {s1:.1f} eps")
    print(f"WORST_SUM_EPS = {max(s for s, _ in ids.values()):.1f}")
    print(f"WORST_MOMENT_EPS = {max(s for _, s in ids.values()):.1f}")

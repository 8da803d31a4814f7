"""Tetrahedron trace of the Green's function, CPU side: the numpy restatement (tests/gltm_numpy.py) against 60-digit
mpmath, a Monte-Carlo mean, the exact DOS and its own limits, and the bindings of abz_rule_ltm_green.  The device kernel is
checked against the same restatement in test_gpu_ltm_green.py."""
import math
import os
import re

import numpy as np
import pytest

import abz_oracle as orc
import gltm_numpy as gn
import ltm_numpy as ln
from test_ltm_cpu import degenerate_bands
from test_oracle_pins import dos_integer_3d_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIVE = [-2.3, -0.6, 0.45, 1.7, 3.1]  # inside the band of tb_integer(3), away from its van Hove points at +-2, +-6

# ---------------------------------------------------------------- 1. restatement against mpmath
MP_CASES = {
    "int3_8": (lambda: orc.tb_integer(3), 8),
    "int2_16": (lambda: orc.tb_integer(2), 16),
    "graphene_12": (orc.tb_graphene, 12),
    "syn4_5": (lambda: orc.synthetic_wannier(4, rmax=1, seed=3), 5),
}
MP_ETAS = [0.3, 1e-2, 1e-4, 1e-8]

# The worst per-simplex relative error of the restatement over all of MP_CASES x MP_ETAS x mp_energies, in units of
# eps = 2^-52, as printed by `PYTHONPATH=oracle python tests/test_ltm_green_cpu.py` (int3_8 60.3, int2_16 18.4, graphene_12 16.1, syn4_5 73.7).
WORST_MEASURED_EPS = 73.7
assert WORST_MEASURED_EPS <= 1e3  # a larger value means the evaluation rule is wrong, not that the bound should grow


def mp_energies(eig):
    lo, hi = float(eig.min()), float(eig.max())
    gamma = eig[(0,) * (eig.ndim - 1)]
    return [lo + 0.37 * (hi - lo), 0.0, hi + 1.0, float(gamma[0])]


def mp_worst(name):
    make, npt = MP_CASES[name]
    eig = ln.grid_eigenvalues(make(), npt)
    e = ln.kuhn_simplices(eig)
    worst = 0.0
    for eta in MP_ETAS:
        for E in mp_energies(eig):
            worst = max(worst, gn.worst_relative_error(e, complex(E, eta)))
    return worst


@pytest.mark.parametrize("name", list(MP_CASES))
def test_restatement_vs_mpmath(name):
    """Per-simplex |J - J_mp| / |J_mp| against the pure recursion at 60 digits; bound 4 x the worst the restatement shows."""
    worst = mp_worst(name)
    print(f"green restatement vs mpmath {name}: worst relative error {worst:.1f} eps (bound {4 * WORST_MEASURED_EPS:.0f})")
    assert worst <= 4 * WORST_MEASURED_EPS, (name, worst)


# ---------------------------------------------------------------- 2. Monte-Carlo check of J
@pytest.mark.parametrize("m", [2, 3])
def test_J_is_the_mean_over_the_simplex(m):
    """J against the mean of 1 / (z - e) over 4e5 uniform points of a random triangle / tetrahedron (e is linear: the
    barycentric coordinates are Dirichlet(1..1)), z = 0.3 + 0.2i; statistical error about 1e-3, bound 1e-2 relative."""
    rng = np.random.default_rng(1234 + m)
    x = np.sort(rng.uniform(-1.0, 1.0, m + 1))
    z = 0.3 + 0.2j
    lam = rng.dirichlet(np.ones(m + 1), size=400_000)
    mc = (1.0 / (z - lam @ x)).mean()
    J = gn.simplex_J(x, z)[0]
    rel = abs(J - mc) / abs(mc)
    print(f"J vs Monte Carlo m={m}: relative deviation {rel:.2e}")
    assert rel <= 1e-2


# ---------------------------------------------------------------- 3. physics
@pytest.fixture(scope="module")
def int3_48():
    """The 48^3 grid of tb_integer(3) and its broadened DOS at FIVE for eta = 1e-3 and 1e-5, computed once."""
    eig = ln.grid_eigenvalues(orc.tb_integer(3), 48)
    e = ln.kuhn_simplices(eig)
    dos = {eta: -gn.green_trace(eig, [complex(E, eta) for E in FIVE], simplices=e).imag / math.pi for eta in (1e-3, 1e-5)}
    return eig, dos


def test_exact_dos_at_small_eta(int3_48):
    """-Im tr G / pi at eta = 1e-3 on 48^3 within 1e-2 of the exact DOS (measured 2.0e-4), where the plain grid mean of the
    same eigenvalues is more than 0.1 off."""
    eig, dos = int3_48
    eta = 1e-3
    exact = np.array([dos_integer_3d_exact(E) for E in FIVE])
    err = np.abs(dos[eta] - exact).max()
    plain = np.array([gn.plain_grid_dos(eig, E, eta) for E in FIVE])
    perr = np.abs(plain - exact).max()
    print(f"eta=1e-3 npt=48: tetrahedron max err {err:.2e}, plain grid mean max err {perr:.2e}")
    assert err <= 1e-2
    assert perr > 0.1


def test_limit_to_eta_zero(int3_48):
    """The broadened DOS tends to g_LTM(E) linearly in eta: the difference at 1e-5 is at most 0.02 x that at 1e-3 (measured 0.01)."""
    eig, dos = int3_48
    g, _ = ln.ltm(eig, FIVE)
    d = {eta: np.abs(dos[eta] - g).max() for eta in (1e-3, 1e-5)}
    print(f"|broadened - g_LTM|: {d[1e-3]:.2e} at eta=1e-3, {d[1e-5]:.2e} at eta=1e-5, ratio {d[1e-5] / d[1e-3]:.3f}")
    assert d[1e-5] <= 0.02 * d[1e-3]


@pytest.mark.parametrize("name", ["int3_8", "syn4_5", "graphene_12"])
def test_large_z(name):
    make, npt = MP_CASES[name]
    eig = ln.grid_eigenvalues(make(), npt)
    n = eig.shape[-1]
    z = 1e8j
    t = gn.green_trace(eig, [z])[0]
    assert abs(z * t - n) <= 1e-6 * n, (z * t, n)


def test_equal_and_nearly_equal_corners():
    """diag(e, e, 0.25) labelled ascending per node (flat pieces, corners exactly and nearly at 0.25) stays finite at
    z = 0.25 + 1e-8i, and agrees with the unsorted labelling, whose flat band is 1 / u exactly; all-equal corners give 1 / u."""
    z = 0.25 + 1e-8j
    a = gn.green_trace(degenerate_bands(8, sort=True), [z])[0]
    b = gn.green_trace(degenerate_bands(8, sort=False), [z])[0]
    assert np.isfinite(a.real) and np.isfinite(a.imag) and np.isfinite(b.real) and np.isfinite(b.imag)
    one = gn.green_trace(ln.grid_eigenvalues(orc.tb_integer(3), 8), [z])[0]
    assert abs(b - (2 * one + 1.0 / (z - 0.25))) <= 1e-12 * abs(b)
    for m in (1, 2, 3):
        for zz in (z, 0.3 + 0.2j, 1e8j, -4.0 + 1e-8j):
            x = np.full(m + 1, 0.25)
            assert gn.simplex_J(x, zz)[0] == (1.0 / (np.array([zz]) - 0.25))[0]  # numpy's own complex reciprocal
        # one ulp apart: the series, close to 1 / u
        x = np.array([0.25] * m + [np.nextafter(0.25, 1.0)])
        J = gn.simplex_J(x, z)[0]
        assert abs(J - 1.0 / (z - 0.25)) <= 1e-7 * abs(J)
    assert gn.simplex_J_any([0.1, 0.2, 0.5, 0.9], 0.3 - 0.2j)[0] == np.conj(gn.simplex_J([0.1, 0.2, 0.5, 0.9], 0.3 + 0.2j)[0])


# ---------------------------------------------------------------- 4. bindings
def test_ltm_green_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    assert "abz_rule_ltm_green" in L.PROTOTYPES
    assert re.search(r"^int abz_rule_ltm_green\(abz_rule\* r, const double\* z(?: /\*.*?\*/)?, int nz, double\* out(?: /\*.*?\*/)?\);", hdr,
                     flags=re.M)
    assert hasattr(L.lib(), "abz_rule_ltm_green")
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert ":abz_rule_ltm_green" in jl
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_K_COUNT"] == 8 and defs["ABZ_VERSION"] == 502
    assert hasattr(abz.DeviceRule, "ltm_green") and hasattr(abz.dos, "green_trace")


def test_ltm_eta_arguments():
    import autobzcore.jl_amd as abz
    assert abz.LTM().eta is None and abz.LTM(npt=7).eta is None
    assert abz.LTM(eta=0.1).eta == 0.1 and abz.LTM(npt=9, eta=1e-3, symmetric=True).symmetric is True
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            abz.LTM(eta=bad)
    for kw in ({"cumulative": True}, {"elements": np.ones((8, 1))}, {"correction": True, "cumulative": True}):
        with pytest.raises(ValueError):
            abz.LTM(eta=0.1, **kw)


def test_ltm_eta_fails_loudly_without_gpu():
    import torch
    import autobzcore.jl_amd as abz
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    bz = abz.load_bz(abz.FBZ(), [[2 * np.pi]])
    with pytest.raises(abz.AbzError):
        abz.dos.init(abz.DOSProblem(h, 0.0, bz), abz.LTM(eta=0.1))


if __name__ == "__main__":  # prints WORST_MEASURED_EPS:  PYTHONPATH=oracle python tests/test_ltm_green_cpu.py
    per = {name: mp_worst(name) for name in MP_CASES}
    for name, w in per.items():
        print(f"{name}: worst per-simplex relative error {w:.1f} eps")
    print(f"WORST_MEASURED_EPS = {max(per.values()):.1f}")

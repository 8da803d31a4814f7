"""Bloechl's curvature correction of the weighted tetrahedron sums, CPU side: the bindings of ABZ_LTM_STATES_CORRECTED, the
argument checks of the Python front end, and the numpy restatement (tests/bloechl_numpy.py) against its own identities
and against what the correction is for -- the band energy at fixed filling.  The device kernel is checked against the
same restatement in test_gpu_ltm_bloechl.py."""
import os
import re

import numpy as np
import pytest

import bloechl_numpy as bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. bindings
def test_bloechl_bindings():
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_LTM_STATES_CORRECTED"] == 2
    assert L.LTM_STATES_CORRECTED == 2
    assert (defs["ABZ_LTM_DOS"], defs["ABZ_LTM_STATES"]) == (L.LTM_DOS, L.LTM_STATES) == (0, 1)
    # no new entry point, no new prototype
    assert re.search(r"^int abz_rule_ltm_weighted\(abz_rule\* r, int source, const double\* E, int nE, int what, double\* out\);", hdr,
                     flags=re.M)
    assert re.search(r"^int abz_rule_ltm\(abz_rule\* r, const double\* E, int nE, int what, double\* out\);", hdr, flags=re.M)
    assert defs["ABZ_K_COUNT"] == 8 and defs["ABZ_VERSION"] == 502
    assert not [name for name in L.PROTOTYPES if "bloechl" in name or "correct" in name]
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert re.search(r"LTM_STATES_CORRECTED\s*=.*Cint\(2\)", jl) and "correction::Bool=false" in jl


# ---------------------------------------------------------------- 2. the Python front end
def test_bloechl_front_end_arguments():
    import inspect
    import autobzcore.jl_amd as abz
    with pytest.raises(ValueError, match="cumulative"):
        abz.LTM(elements="energy", correction=True)
    with pytest.raises(ValueError, match="elements"):
        abz.LTM(cumulative=True, correction=True)
    alg = abz.LTM(cumulative=True, elements="energy", correction=True)
    assert alg.correction is True and alg.cumulative is True and alg.elements == "energy"
    assert abz.LTM().correction is False and abz.LTM(cumulative=True, elements="energy").correction is False
    assert abz.LTM(cumulative=True, elements="orbitals", eigenvectors="device", correction=True).correction
    assert abz.LTM(cumulative=True, elements="energy", symmetric=True, correction=True).symmetric
    assert callable(abz.dos.band_energy)
    sig = inspect.signature(abz.dos.band_energy)
    assert list(sig.parameters) == ["prob_or_cache", "nstates", "tol", "correction"]
    assert sig.parameters["correction"].default is True and sig.parameters["tol"].default == 1e-10
    ltm = inspect.signature(abz.DeviceRule.ltm)
    assert list(ltm.parameters) == ["self", "Es", "states", "elements", "correction"] and ltm.parameters["correction"].default is False


# ---------------------------------------------------------------- 3. identities of the restatement
MODELS = {
    1: dict(npt=37, d=1),
    2: dict(npt=13, d=2, t=(1.0, 0.7, 0.0), diag=0.5),
    3: dict(npt=6, d=3, t=(1.0, 0.8, 0.6), diag=0.5),
}


def energies(eig):
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    return np.concatenate([np.linspace(lo + 0.02 * w, hi - 0.02 * w, 23), [eig.reshape(-1)[1]]])


def test_factor():
    assert (bn.factor(1), bn.factor(2), bn.factor(3)) == (1.0 / 12.0, 1.0 / 24.0, 1.0 / 40.0)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_correction_of_the_plain_state_count_is_zero(d):
    """kappa_T = f_d sum_i (sum_l e_l - (d+1) e_i) = 0 for A = 1: to rounding of the d + 1 terms, |kappa_T| <= 4 ulp of the band
    width, and the sum w sum_T g_T kappa_T stays below 1e-14."""
    eig = bn.cosine_band(**MODELS[d])
    Es = energies(eig)
    c = bn.correction(eig, np.ones_like(eig), Es)
    print(f"d={d}: max |correction of A = 1| = {np.abs(c).max():.2e}")
    assert c.shape == (len(Es), 1) and np.abs(c).max() <= 1e-14


@pytest.mark.parametrize("d", [1, 2, 3])
def test_correction_is_linear_in_the_elements(d):
    eig = bn.cosine_band(**MODELS[d])
    Es = energies(eig)
    rng = np.random.default_rng(5)
    A1, A2 = rng.standard_normal((2,) + eig.shape)
    c = bn.correction(eig, np.stack([A1, A2, 2.0 * A1 - 3.0 * A2]), Es)
    assert np.abs(c[:, :2]).max() > 1e-4  # something to compare
    dev = np.abs(c[:, 2] - (2.0 * c[:, 0] - 3.0 * c[:, 1])).max()
    print(f"d={d}: linearity {dev:.2e}")
    assert dev <= 1e-13 * max(1.0, np.abs(c).max())


@pytest.mark.parametrize("d", [1, 2, 3])
def test_correction_vanishes_outside_the_bands(d):
    eig = bn.cosine_band(**MODELS[d])
    lo, hi = float(eig.min()), float(eig.max())
    A = np.random.default_rng(5).standard_normal((2,) + eig.shape)
    c = bn.correction(eig, A, [lo - 1.0, np.nextafter(lo, -np.inf), hi, hi + 1.0])
    assert np.all(c == 0.0)


# ---------------------------------------------------------------- 4. what the correction is for
@pytest.fixture(scope="module")
def reference_band_energy():
    """the corrected restatement at 64^3, filling 0.30 of -2 (cos k1 + cos k2 + cos k3)"""
    return bn.band_energy(bn.cosine_band(64), 0.30)[0]


@pytest.mark.parametrize("npt", [8, 12, 16])
def test_corrected_band_energy_converges_faster(npt, reference_band_energy):
    """Band energy at filling 0.30, E_F by bisection on the grid's own plain N(E): the corrected error is at most a fifth of
    the plain one.  The factor 5 is a condition; the restatement gives 17.8 / 5220 / 31 at npt 8 / 12 / 16."""
    eig = bn.cosine_band(npt)
    plain = bn.band_energy(eig, 0.30, corrected=False)[0] - reference_band_energy
    corr = bn.band_energy(eig, 0.30, corrected=True)[0] - reference_band_energy
    print(f"npt={npt}: band-energy error plain {plain:+.3e}, corrected {corr:+.3e}, ratio {abs(plain) / abs(corr):.1f}")
    assert abs(corr) <= abs(plain) / 5.0

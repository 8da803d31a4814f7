"""Tetrahedron method with matrix elements, CPU side: the geometric restatement (tests/wltm_numpy.py) against the
shipped restatement of the unweighted method, its own sum rules and an analytic band energy; and the bindings of
abz_rule_ltm_elements / abz_rule_ltm_weighted / abz_rule_ltm_fermi.  The device kernels are checked against the same
restatement in test_gpu_ltm_weighted.py."""
import math
import os
import re

import numpy as np
import pytest

import ltm_numpy as ln
import wltm_numpy as wn
from test_ltm_cpu import MODELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRIDS = [("int1", 48), ("int2", 12), ("graphene", 10), ("int3", 6)]


def energies(eig):
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    return np.concatenate([np.linspace(lo - 0.05 * w, hi + 0.05 * w, 41), eig.reshape(-1)[:3]])


def bound(ref):
    return 1e-12 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("name,npt", GRIDS)
def test_weighted_restatement_with_unit_elements_is_the_plain_method(name, npt):
    eig = ln.grid_eigenvalues(MODELS[name][0](), npt)
    Es = energies(eig)
    g_ref, N_ref = ln.ltm(eig, Es)
    g, N = wn.wltm(eig, np.ones_like(eig), Es)
    assert g.shape == N.shape == (len(Es), 1)
    dg, dN = np.abs(g[:, 0] - g_ref).max(), np.abs(N[:, 0] - N_ref).max()
    print(f"{name} npt={npt}: A = 1 against ltm_numpy: g {dg:.2e} (bound {bound(g_ref):.1e}), N {dN:.2e} (bound {bound(N_ref):.1e})")
    assert dg <= bound(g_ref) and dN <= bound(N_ref)


@pytest.mark.parametrize("name,npt", GRIDS)
def test_weighted_restatement_with_the_energy_as_element(name, npt):
    """A = e is linear in the simplex like e itself, so g_e(E) = E g(E); above all bands N_A is the sum over bands of
    the mean of A over the nodes (every node is a corner of the same number of simplices)."""
    eig = ln.grid_eigenvalues(MODELS[name][0](), npt)
    Es = energies(eig)
    g_ref, _ = ln.ltm(eig, Es)
    rng = np.random.default_rng(3)
    A = np.stack([eig, rng.standard_normal(eig.shape)])
    g, N = wn.wltm(eig, A, Es)
    dev = np.abs(g[:, 0] - Es * g_ref).max()
    print(f"{name} npt={npt}: g_e - E g {dev:.2e} (bound {bound(Es * g_ref):.1e})")
    assert dev <= bound(Es * g_ref)
    top = int(np.argmax(Es))
    assert Es[top] > eig.max()
    total = A.reshape(2, -1, eig.shape[-1]).mean(axis=1).sum(axis=1)
    dtop = np.abs(N[top] - total).max()
    print(f"{name} npt={npt}: N_A above the bands - sum_b mean_k A_b: {dtop:.2e}")
    assert dtop <= 1e-12
    assert np.all(g[top] == 0.0) and np.all(N[int(np.argmin(Es))] == 0.0)


def test_band_energy_of_the_half_filled_cosine_band():
    """The 1-D band 2 cos 2 pi k at E = 0 with A = e: N_e(0) = int_{1/4}^{3/4} 2 cos 2 pi k dk = -2 / pi, the band energy
    at half filling.  The linear interpolation is second order: measured with the prototype of this restatement
    8.4e-4 / 2.1e-4 / 5.2e-5 at npt 50 / 100 / 200, i.e. 2.1 / npt^2; bound 2e-4 at npt 200 (4 x the measured figure:
    the constant was measured on this one model), and the ratio between npt 100 and 200 within 3.5 ... 4.5."""
    import abz_oracle as orc
    exact = -2.0 / math.pi
    err = {}
    for npt in (100, 200):
        eig = ln.grid_eigenvalues(orc.tb_integer(1), npt)
        _, N = wn.wltm(eig, eig, np.array([0.0]))
        err[npt] = abs(N[0, 0] - exact)
        print(f"npt={npt}: N_e(0) + 2/pi = {N[0, 0] - exact:.3e}")
    assert err[200] <= 2e-4
    assert 3.5 <= err[100] / err[200] <= 4.5, err


def test_weighted_ltm_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    protos = {
        "abz_rule_ltm_elements": r"^int abz_rule_ltm_elements\(abz_rule\* r, const double\* A, int ncomp\);",
        "abz_rule_ltm_weighted": r"^int abz_rule_ltm_weighted\(abz_rule\* r, int source, const double\* E, int nE, int what, double\* out\);",
        "abz_rule_ltm_fermi": r"^int abz_rule_ltm_fermi\(abz_rule\* r, double nstates, double tol, double\* E_F, double\* N_F\);",
    }
    for name, rx in protos.items():
        assert re.search(rx, hdr, flags=re.M), name
        assert name in L.PROTOTYPES, name
        assert hasattr(L.lib(), name), name
        assert ":" + name in jl, name
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_LTM_MAX_COMP"] == L.LTM_MAX_COMP == 16
    assert (defs["ABZ_LTM_A_ELEMENTS"], defs["ABZ_LTM_A_ENERGY"]) == (L.LTM_A_ELEMENTS, L.LTM_A_ENERGY) == (0, 1)
    assert defs["ABZ_K_COUNT"] == 8 and defs["ABZ_VERSION"] == 502
    # abz_rule_ltm itself is as it was
    assert re.search(r"^int abz_rule_ltm\(abz_rule\* r, const double\* E, int nE, int what, double\* out\);", hdr, flags=re.M)
    for meth in ("ltm", "ltm_elements", "ltm_fermi"):
        assert hasattr(abz.DeviceRule, meth), meth
    assert callable(abz.dos.fermi_level)
    alg = abz.LTM()
    assert alg.elements is None and alg.npt == 50 and alg.cumulative is False
    assert abz.LTM(elements="orbitals").elements == "orbitals" and abz.LTM(elements="energy", cumulative=True).cumulative
    f = lambda x, eig: eig[None]
    assert abz.LTM(elements=f).elements is f
    with pytest.raises(ValueError):
        abz.LTM(elements="bands")

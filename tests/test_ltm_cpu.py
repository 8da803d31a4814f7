"""Linear tetrahedron method, CPU side: the numpy restatement (tests/ltm_numpy.py) against the reference's exact DOS
formulas and its own sum rules, and the bindings of abz_rule_ltm.  The device kernel is checked against the same
restatement in test_gpu_ltm.py."""
import os
import re

import numpy as np
import pytest

import abz_oracle as orc
import ltm_numpy as ln
from test_oracle_pins import dos_graphene_exact, dos_integer_1d_exact, dos_integer_2d_exact, dos_integer_3d_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODELS = {
    "int1": (lambda: orc.tb_integer(1), dos_integer_1d_exact, 2),
    "int2": (lambda: orc.tb_integer(2), dos_integer_2d_exact, 4),
    "graphene": (orc.tb_graphene, dos_graphene_exact, 4),
    "int3": (lambda: orc.tb_integer(3), dos_integer_3d_exact, 6),
}


def reference_energies(B):
    # ref: test/dos.jl:105
    return [-B - 1, -0.8 * B, -0.6 * B, -0.2 * B, 0.1 * B, 0.3 * B, 0.5 * B, 0.7 * B, 0.9 * B, B + 2]


@pytest.mark.parametrize("name,npt", [("int1", 200), ("int2", 200), ("graphene", 200), ("int3", 48)])
def test_restatement_vs_exact_dos(name, npt):
    """ref: test/dos.jl:88-111 with the restatement in the place of GGR, atol 1e-2 (measured: 3.3e-3, 8.6e-5, 7.1e-4, 2.3e-4)."""
    make, exact, B = MODELS[name]
    Es = reference_energies(B)
    g, _ = ln.ltm(ln.grid_eigenvalues(make(), npt), Es)
    err = [abs(u - exact(e)) for u, e in zip(g, Es)]
    print(name, npt, "max |g - exact| =", max(err))
    assert max(err) < 1e-2, (name, npt, err)


@pytest.mark.parametrize("name,npt", [("int1", 64), ("int2", 32), ("graphene", 32), ("int3", 16)])
def test_restatement_state_count_sum_rules(name, npt):
    """N is exactly 0 below the bands, n to 1e-12 n above them (the reference's TODO 'integrate to unity'), non-decreasing."""
    make, _, B = MODELS[name]
    eig = ln.grid_eigenvalues(make(), npt)
    n = eig.shape[-1]
    Es = np.linspace(-B - 1.0, B + 2.0, 257)
    g, N = ln.ltm(eig, Es)
    assert N[0] == 0.0 and g[0] == 0.0 and g[-1] == 0.0
    assert abs(N[-1] - n) <= 1e-12 * n, (N[-1], n)
    assert np.all(np.diff(N) >= 0.0)
    assert np.all(g >= 0.0)


def test_restatement_state_count_is_the_integral_of_the_dos():
    """Cumulative trapezoid of g on linspace(-6.5, 6.5, 1301) against N, 3-D model at npt 16: the trapezoid's quadrature
    error on a piecewise-quadratic g (measured 1.9e-6), bound 1e-5."""
    eig = ln.grid_eigenvalues(orc.tb_integer(3), 16)
    Es = np.linspace(-6.5, 6.5, 1301)
    g, N = ln.ltm(eig, Es)
    trap = np.concatenate([[0.0], np.cumsum(0.5 * (g[1:] + g[:-1]) * np.diff(Es))])
    dev = np.abs(trap - N).max()
    print("max |cumtrapz(g) - N| =", dev)
    assert dev < 1e-5


def degenerate_bands(npt=8, sort=False):
    """Two copies of the 3-D band and a constant band at 0.25 [npt, npt, npt, 3]; `sort`: ascending per node, the labels an
    eigensolver gives the same spectrum."""
    e = ln.grid_eigenvalues(orc.tb_integer(3), npt)[..., 0]
    bands = np.stack([e, e, np.full_like(e, 0.25)], axis=-1)
    return np.sort(bands, axis=-1) if sort else bands


def test_restatement_flat_and_degenerate_bands():
    """Every simplex of the constant band is flat (all corners equal): it gives nothing to g, also at E = 0.25 itself,
    and a unit step to N there; the two equal bands give twice the single band."""
    npt = 8
    one = ln.grid_eigenvalues(orc.tb_integer(3), npt)
    below = np.nextafter(0.25, -1.0)
    Es = np.array([-7.0, -1.0, below, 0.25, 0.3, 7.0])
    g, N = ln.ltm(degenerate_bands(npt), Es)
    g1, N1 = ln.ltm(one, Es)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(N))
    flat_step = (Es >= 0.25).astype(float)
    assert np.abs(g - 2 * g1).max() <= 1e-12 * max(1.0, g.max()), (g, g1)
    assert np.abs(N - (2 * N1 + flat_step)).max() <= 1e-12 * 3
    jump = N[3] - N[2]
    print("N(0.25) - N(0.25 - ulp) =", jump)
    assert abs(jump - 1.0) <= 1e-12
    assert N[0] == 0.0 and abs(N[-1] - 3.0) <= 3e-12
    # the same spectrum labelled ascending per node (what the device's eigensolver hands the kernel): bands 0 and 2 are
    # min(e, 0.25) and max(e, 0.25) with flat pieces and corners exactly at 0.25; finite, same sum rules
    gs, Ns = ln.ltm(degenerate_bands(npt, sort=True), np.sort(np.concatenate([Es, np.linspace(-6.5, 6.5, 53)])))
    assert np.all(np.isfinite(gs)) and np.all(np.isfinite(Ns)) and np.all(gs >= 0.0)
    assert Ns[0] == 0.0 and abs(Ns[-1] - 3.0) <= 3e-12 and np.all(np.diff(Ns) >= 0.0)


# ---------------------------------------------------------------- bindings
def test_ltm_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    assert issubclass(abz.LTM, abz.dos.DOSAlgorithm)
    alg = abz.LTM()
    assert alg.npt == 50 and alg.cumulative is False
    assert abz.LTM(npt=7, cumulative=True).cumulative is True
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    assert "abz_rule_ltm" in L.PROTOTYPES
    assert re.search(r"^int abz_rule_ltm\(abz_rule\* r, const double\* E, int nE, int what, double\* out\);", hdr, flags=re.M)
    assert hasattr(L.lib(), "abz_rule_ltm")
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert ":abz_rule_ltm" in jl
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert (defs["ABZ_LTM_DOS"], defs["ABZ_LTM_STATES"]) == (L.LTM_DOS, L.LTM_STATES) == (0, 1)
    assert defs["ABZ_K_LTM"] == L.K_LTM == 6
    assert defs["ABZ_K_COUNT"] == 8 and defs["ABZ_VERSION"] == 502
    assert hasattr(abz.DeviceRule, "ltm")


def test_ltm_fails_loudly_without_gpu():
    import torch
    import autobzcore.jl_amd as abz
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    bz = abz.load_bz(abz.FBZ(), [[2 * np.pi]])
    with pytest.raises(abz.AbzError):
        abz.dos.init(abz.DOSProblem(h, 0.0, bz), abz.LTM())

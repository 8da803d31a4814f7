"""Complex integration weights W_b(k; z) of the optimized tetrahedron method without a GPU: the scatter-form restatement of
tests/goptnodew_numpy.py against the sums of goptltm_numpy.green, its exact properties, the conditioning of the device test's
parity cases, the bindings and the refusals the Python front end makes before a device is asked for anything.

The cases, values of z and calls of test_gpu_ltm_green_node_weights_optimized.py are defined here and imported there."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import gnodew_numpy as gnw
import goptltm_numpy as gon
import goptnodew_numpy as gonw
import optltm_numpy as on
import optnodew_numpy as onw
from test_ltm_optimized_cpu import SEEDS, case_coefficients

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EPS = 2.0**-52

# the parity cases of the device test: (model, npt).  npt = 1, 2, 3: the stencil on itself, wrapped planes coincide; 4, 5: the first
# grids on which they do not; 33 bands: more bands than a row of the block holds columns; "flat": one band, 0.25 to the bit.
PARITY_CASES = [(n, npt) for n in (1, 3, 6) for npt in (1, 2, 3, 4, 5)] + [(33, 3), ("svo", 6), ("flat", 3)]


def model_coefficients(n):
    """case_coefficients of test_ltm_optimized_cpu.py, continued to band counts it has no seed for"""
    if n in SEEDS:
        return case_coefficients(n)
    rng = np.random.default_rng(101 * n)
    c = rng.standard_normal((3, 3, 3, n, n)) + 1j * rng.standard_normal((3, 3, 3, n, n))
    return 0.5 * (c + np.conj(np.swapaxes(c[::-1, ::-1, ::-1], -1, -2))), (-1, -1, -1)


def model_series(abz, model):
    if model == "svo":
        return abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    if model == "flat":
        c = np.zeros((3, 3, 3, 1, 1), dtype=np.complex128)
        c[1, 1, 1, 0, 0] = 0.25
        return abz.FourierSeries(c, period=1.0, first=(-1, -1, -1), ndim=3)
    c, first = model_coefficients(model)
    return abz.FourierSeries(c, period=1.0, first=first, ndim=3)


def model_eigenvalues(model, npt):
    import abz_oracle as orc
    import autobzcore.jl_amd as abz
    import ltm_numpy as ln
    if model == "flat":
        return np.full((npt, npt, npt, 1), 0.25)
    s = model_series(abz, model)
    return ln.grid_eigenvalues(orc.FourierSeries(s.c, period=1.0, first=tuple(s.first), ndim=3), npt)


def z_pool(eig):
    """28 values: goptltm_numpy.z_lists' 20 generic ones (position 5 y + x: Im z = 0.5, 1e-2, 1e-4, -1e-3 for y = 0..3; Re z below the
    bands, three inside, above for x = 0..4), then its 8 "edges" (effective corner values of the grid + 1e-8j)."""
    zl = gon.z_lists(eig)
    return np.concatenate([zl["generic"], zl["edges"]])


def calls_for(model, npt):
    """label -> positions in z_pool: calls of 1, 3 and 8 values, unsorted, one value twice.  At npt = 1 and on the exactly flat band
    W = 1 / (z - e') and an ulp of e' moves it by ulp / eta^2: |Im z| >= 1e-3 only there, and no edges."""
    if npt == 1 or model == "flat":
        return {"one": [7], "three": [16, 3, 8], "eight": [19, 0, 6, 7, 2, 15, 7, 4]}
    return {"one": [7], "three": [21, 16, 12], "eight": [19, 0, 11, 7, 2, 15, 7, 13], "edges": list(range(20, 28))}


def z_six(eig):
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo if hi > lo else 1.0
    flat = eig.reshape(-1)
    return np.array([lo + 0.37 * w + 0.5j, lo + 0.52 * w + 1e-2j, lo + 0.71 * w + 1e-4j, lo + 0.13 * w - 1e-3j, hi + 0.3 * w + 0.2j,
                     flat[(7 * len(flat)) // 11] + 1e-8j])


# ---------------------------------------------------------------- 1. bindings (fails without the feature)
def test_green_node_weights_optimized_bindings():
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    assert re.search(r"^int abz_rule_ltm_green_node_weights_optimized\(abz_rule\* r, const double\* z /\* \[nz\]\[2\] \*/, int nz, "
                     r"double\* out /\* \[nz\]\[nk\]\[n\]\[2\] or NULL \*/\);", hdr, flags=re.M)
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_VERSION"] == 502 and defs["ABZ_K_COUNT"] == 8 and defs["ABZ_LTM_GREEN_NODEW_MAX_Z"] == 8
    assert L.PROTOTYPES["abz_rule_ltm_green_node_weights_optimized"] == L.PROTOTYPES["abz_rule_ltm_green_node_weights"]
    assert hasattr(L.lib(), "abz_rule_ltm_green_node_weights_optimized")  # the built library exports it
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert ":abz_rule_ltm_green_node_weights_optimized" in jl and "function ltm_green_node_weights_optimized(" in jl
    mk = open(os.path.join(ROOT, "autobzcore.jl_amd", "csrc", "Makefile")).read()
    assert "kernels_ltm_green_opt_nodew.o" in mk and "kernels_ltm_green_opt_nodew.hip" in mk and "ltm_opt_nodew_device.h" in mk
    # a null handle and a null z are refused before anything else is looked at
    assert L.lib().abz_rule_ltm_green_node_weights_optimized(None, None, 1, None) == L.ERR_ARG
    assert b"null rule handle" in L.lib().abz_last_error()


def test_green_node_weights_optimized_signatures():
    import autobzcore.jl_amd as abz
    sig = inspect.signature(abz.DeviceRule.ltm_green_node_weights_optimized).parameters
    assert list(sig) == ["self", "zs", "export"] and sig["export"].default is True
    for f, names in ((abz.DeviceRule.ltm_green_node_weights_matrix, ["self", "zs", "orbitals", "optimized"]),
                     (abz.dos.green_weights, ["prob_or_cache", "zs", "fold", "optimized"]),
                     (abz.dos.green_local_fused, ["prob_or_cache", "zs", "orbitals", "optimized"])):
        p = inspect.signature(f).parameters
        assert list(p) == names and p["optimized"].default is False, f
    assert list(inspect.signature(abz.dos.green_local).parameters) == ["prob_or_cache", "zs", "orbitals"]
    assert list(inspect.signature(abz.DeviceRule.ltm_green_matrix).parameters) == ["self", "zs", "orbitals"]


# ---------------------------------------------------------------- 2. identities of the restatement
@pytest.mark.parametrize("n", (1, 2, 3))
@pytest.mark.parametrize("npt", (2, 3, 4, 5))
def test_weights_give_the_sums_of_the_optimized_green_functions(n, npt):
    """sum W = tr G, sum W A = G_A for 3 random components and sum W e = the energy-weighted G (= z tr G - n) of goptltm_numpy.green.
    Bound 1e-12 max(1, |ref|): at most 6 x 125 x 3 x 20 terms per sum."""
    eig = model_eigenvalues(n, npt)
    zs = z_six(eig)
    A = np.random.default_rng(10 * n + npt).standard_normal((3,) + eig.shape)
    W = gonw.node_weights(eig, zs)
    tr = gon.green(eig, None, zs)
    for label, got, ref in (("sum W against tr G", W.sum(axis=(1, 2, 3, 4)), tr),
                            ("sum W A against G_A", np.einsum("zxyub,cxyub->zc", W, A), gon.green(eig, A, zs)),
                            ("sum W e against the energy-weighted G", np.einsum("zxyub,xyub->z", W, eig), gon.green(eig, "energy", zs)[:, 0]),
                            ("sum W e against z tr G - n", np.einsum("zxyub,xyub->z", W, eig), zs * tr - n)):
        dev = float(np.abs((got - ref) / np.maximum(1.0, np.abs(ref))).max())
        print(f"n={n} npt={npt} {label}: {dev:.2e} of max(1, |ref|)")
        assert dev <= 1e-12, label


@pytest.mark.parametrize("n,npt", [(1, 2), (3, 3), (2, 5)])
def test_conjugate_z_gives_the_conjugate_weights_to_the_bit(n, npt):
    eig = model_eigenvalues(n, npt)
    zs = z_six(eig)
    a, b = gonw.node_weights(eig, zs), gonw.node_weights(eig, np.conj(zs))
    assert np.array_equal(np.conj(a).view(np.uint64), b.view(np.uint64))


def test_a_flat_band_weighs_every_node_alike():
    """e = e0 everywhere: every e' is e0 to the bit, every corner weight 1 / (4 (z - e0)), and a node sums 432 signed terms whose
    coefficients add up to nk x 24: nk W = 1 / (z - e0) within 432 eps relative."""
    e0, z, npt = 0.25, 0.1 + 0.3j, 3
    W = gonw.node_weights(np.full((npt, npt, npt, 1), e0), [z])[0]
    dev = float(np.abs(npt ** 3 * W - 1.0 / (z - e0)).max()) * abs(z - e0)
    print(f"flat band: |nk W - 1 / (z - e0)| = {dev / EPS:.2f} eps relative")
    assert dev <= 432 * EPS


def test_weights_tend_to_the_dos_weights():
    """-Im W(E + i eta) / pi -> the DOS weights of optnodew_numpy, linearly in eta: the deviation falls by 100 +- 10 % per factor 100."""
    npt, E = 5, -1.3
    eig = on.issue_band(npt)
    w = onw.node_weights(eig, [E], states=False)[0]
    etas = [1e-3, 1e-5, 1e-7]
    W = gonw.node_weights(eig, [E + 1j * eta for eta in etas])
    dev = [float(np.abs(npt ** 3 * (-W[i].imag / np.pi - w)).max()) for i in range(3)]
    print("eta -> 0: nk |-Im W / pi - w_dos| = " + ", ".join(f"{d:.3e} at {eta:g}" for d, eta in zip(dev, etas)))
    for a, b in zip(dev, dev[1:]):
        assert 90.0 <= a / b <= 110.0, dev


def test_optimized_weights_are_not_the_linear_weights():
    eig = model_eigenvalues(3, 5)
    zs = z_six(eig)[:4]
    diff = float(np.abs(125 * (gonw.node_weights(eig, zs) - gnw.node_weights(eig, zs))).max())
    print(f"npt = 5: max |nk (W_opt - W_lin)| = {diff:.3e}")
    assert diff > 1e-2


# ---------------------------------------------------------------- 3. conditioning of the device test's parity cases
@pytest.mark.parametrize("model,npt", PARITY_CASES, ids=[f"{m}-{p}" for m, p in PARITY_CASES])
def test_device_cases_are_well_conditioned(model, npt):
    """The f64 and the longdouble product of the 20 points through the same closed forms, at every value of z the device test
    calls: they differ by at most 0.01 of its parity bound 1e-9 max(1, max|nk ref|), on the real and on the imaginary part, so
    that the bound is a statement about the kernel.  A condition on the choice of cases, not a measurement of the kernel."""
    eig = model_eigenvalues(model, npt)
    pool = z_pool(eig)
    nk = npt ** 3
    used = sorted({i for pick in calls_for(model, npt).values() for i in pick})
    u, v = nk * gonw.node_weights(eig, pool[used]), nk * gonw.node_weights(eig, pool[used], dtype=np.longdouble)
    assert np.all(np.isfinite(u.view(np.float64)))
    worst = 0.0
    for i in range(len(used)):
        scale = max(1.0, float(np.abs(v[i].real).max()), float(np.abs(v[i].imag).max()))
        worst = max(worst, max(float(np.abs(u[i].real - v[i].real).max()), float(np.abs(u[i].imag - v[i].imag).max())) / scale)
    print(f"{model} npt={npt}: f64 against longdouble nk W, worst {worst:.2e} of max(1, max|nk ref|) per z")
    assert worst <= 1e-11


# ---------------------------------------------------------------- 4. refusals of the front end that need no device
def test_front_end_refusals_before_a_device_is_asked():
    import autobzcore.jl_amd as abz
    c, first = case_coefficients(3)
    s = abz.FourierSeries(c, period=1.0, first=first, ndim=3)
    prob = abz.DOSProblem(s, 0.0, abz.load_bz(abz.FBZ(), np.eye(3)))
    z = 0.3 + 0.1j
    # optimized=True makes the weights of zs: the resident ones are what the call that made them says
    stub = types.SimpleNamespace(_ltm_refuse_shard=lambda what=None: None)  # (a rule that is not sharded; nothing else is read)
    with pytest.raises(ValueError, match="optimized=True"):
        abz.DeviceRule.ltm_green_node_weights_matrix(stub, None, None, optimized=True)
    # d < 3
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    prob1 = abz.DOSProblem(h, 0.3, abz.load_bz(abz.FBZ(), [[2 * np.pi]]))
    with pytest.raises(NotImplementedError, match="d = 3"):
        abz.dos.green_weights(prob1, z, optimized=True)
    with pytest.raises(NotImplementedError, match="d = 3"):
        abz.dos.green_local_fused(prob1, [z], optimized=True)
    # fold=True off a symmetric cache
    with pytest.raises(ValueError, match="fold"):
        abz.dos.green_weights(prob, z, fold=True, optimized=True)
    with pytest.raises(ValueError, match="real value"):
        abz.dos.green_weights(prob, 0.3, optimized=True)

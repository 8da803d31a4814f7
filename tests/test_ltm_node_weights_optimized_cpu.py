"""Integration weights of the optimized tetrahedron method, CPU side: the scatter-form restatement of tests/optnodew_numpy.py
against the sums of optltm_numpy.py, its conditioning on the cases of the device test, what distinguishes these weights from
Bloechl's, the bindings of abz_rule_ltm_node_weights_optimized and the argument checks of the Python front end.  The device
kernels are checked against the same restatement in test_gpu_ltm_node_weights_optimized.py."""
import inspect
import os
import re

import numpy as np
import pytest

import nodew_numpy as nw
import optltm_numpy as on
import optnodew_numpy as onw
from test_ltm_optimized_cpu import GRIDS, SEEDS, case_coefficients, case_elements

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the grids of the device's parity test: the stencil on itself (1, 2, 3), GRIDS, and a row padded to 32 with a ragged last block
DEVICE_GRIDS = {1: (1, 2) + GRIDS, 3: (1, 2) + GRIDS + (17,)}


def case_eigenvalues(n, npt):
    import abz_oracle as orc
    import ltm_numpy as ln
    c, first = case_coefficients(n)
    return ln.grid_eigenvalues(orc.FourierSeries(c, period=1.0, first=first, ndim=3), npt)


def energy_list(eig):
    """16 energies in no order: below and above every e' (which leave the eigenvalues' range by less than 0.23 of its width),
    the exact eigenvalue of a node, random ones inside the bands, one of them twice."""
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo if hi > lo else 1.0
    flat = eig.reshape(-1)
    inside = lo + w * np.random.default_rng(5).random(12)
    return np.concatenate([[lo - 0.3 * w, hi + 0.3 * w, flat[(7 * len(flat)) // 11]], inside, inside[:1]])


# the calls of 1, 5 and 16 energies (a single one; a group of 4 and a remainder; four groups): positions in energy_list
CALLS = {1: [8], 5: [9, 1, 2, 0, 9], 16: list(range(16))}


# ---------------------------------------------------------------- 1. identity with the sums
@pytest.mark.parametrize("n", sorted(SEEDS))
@pytest.mark.parametrize("npt", GRIDS)
def test_weights_give_the_sums_of_the_optimized_rule(n, npt):
    """sum_k sum_b W A = the N_A / g_A of optltm for A = 1, A = e and 5 random components: A' = P A, by algebra."""
    eig = case_eigenvalues(n, npt)
    A = case_elements(n, npt).reshape((5,) + eig.shape)
    Es = energy_list(eig)
    for states in (False, True):
        W = onw.node_weights(eig, Es, states)
        for label, arg, contracted in (("one", None, W.sum(axis=(1, 2, 3, 4))[:, None]),
                                       ("energy", "energy", np.einsum("exyzb,xyzb->e", W, eig)[:, None]),
                                       ("elements", A, np.einsum("exyzb,cxyzb->ec", W, A))):
            ref = on.optltm(eig, arg, Es, states)
            dev, scale = float(np.abs(contracted - ref).max()), max(1.0, float(np.abs(ref).max()))
            print(f"n={n} npt={npt} states={states} {label}: |sum W A - optltm| = {dev:.2e} (scale {scale:.2e})")
            assert dev <= 1e-12 * scale


# ---------------------------------------------------------------- 2. conditioning of the device cases
@pytest.mark.parametrize("n,npt", [(n, npt) for n in sorted(DEVICE_GRIDS) for npt in DEVICE_GRIDS[n]])
def test_device_cases_are_well_conditioned(n, npt):
    """f64 against longdouble in nk w at the grids and energies of the device test, so that the device's 1e-9 is a statement
    about the kernel."""
    eig = case_eigenvalues(n, npt)
    Es = energy_list(eig)
    nk = npt ** 3
    for states in (False, True):
        u = onw.node_weights(eig, Es, states)
        v = onw.node_weights(eig, Es, states, dtype=np.longdouble)
        dev = float(np.abs(nk * (u - v)).max()) / max(1.0, float(np.abs(nk * v).max()))
        print(f"n={n} npt={npt} states={states}: f64 against longdouble nk w {dev:.2e} of the scale")
        assert dev <= 1e-10


def test_exact_values_of_the_restatement():
    eig = case_eigenvalues(3, 5)
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    Es = np.array([lo - 0.3 * w, hi + 0.3 * w])
    S, G = onw.node_weights(eig, Es, True), onw.node_weights(eig, Es, False)
    assert np.all(S[0] == 0.0) and np.all(G == 0.0)
    assert np.abs(125 * S[1] - 1.0).max() <= 1e-13


# ---------------------------------------------------------------- 3. another rule
def test_optimized_weights_are_not_the_linear_weights():
    eig = case_eigenvalues(3, 8)
    lo, hi = float(eig.min()), float(eig.max())
    Es = lo + (hi - lo) * np.array([0.3, 0.5, 0.7])
    nk = 8 ** 3
    for states, kind in ((True, "states"), (False, "dos")):
        W, lin = onw.node_weights(eig, Es, states), nw.node_weights(eig, Es, kind)
        print(f"{kind}: max |nk (w_opt - w_lin)| = {nk * np.abs(W - lin).max():.3e}, min nk w_opt = {nk * W.min():.3e}, min nk w_lin = {nk * lin.min():.3e}")
        assert nk * np.abs(W - lin).max() > 1e-3
        assert lin.min() >= 0.0 and W.min() < 0.0  # not confined to [0, 1 / nk]


# ---------------------------------------------------------------- 4. bindings
def test_node_weights_optimized_bindings():
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    assert re.search(r"^int abz_rule_ltm_node_weights_optimized\(abz_rule\* r, const double\* E, int nE, int what, double\* out "
                     r"/\* \[nE\]\[nk\]\[n\] or NULL \*/\);", hdr, flags=re.M)
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_VERSION"] == 502 and defs["ABZ_K_COUNT"] == 8
    assert L.PROTOTYPES["abz_rule_ltm_node_weights_optimized"] == L.PROTOTYPES["abz_rule_ltm_node_weights"]
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert ":abz_rule_ltm_node_weights_optimized" in jl and "function ltm_node_weights_optimized(" in jl
    mk = open(os.path.join(ROOT, "autobzcore.jl_amd", "csrc", "Makefile")).read()
    assert "kernels_ltm_opt_nodew.o" in mk and "kernels_ltm_opt_nodew.hip" in mk
    # a null handle is refused before anything else is looked at
    assert L.lib().abz_rule_ltm_node_weights_optimized(None, None, 1, L.LTM_STATES, None) == L.ERR_ARG
    assert b"null rule handle" in L.lib().abz_last_error()


# ---------------------------------------------------------------- 5. the Python front end
def test_node_weights_optimized_front_end_arguments():
    import autobzcore.jl_amd as abz
    assert list(inspect.signature(abz.DeviceRule.ltm_node_weights_optimized).parameters) == ["self", "Es", "states", "export"]
    sig = inspect.signature(abz.DeviceRule.ltm_node_weights_optimized).parameters
    assert sig["states"].default is True and sig["export"].default is True
    dm = inspect.signature(abz.DeviceRule.ltm_density_matrix).parameters
    assert list(dm) == ["self", "Es", "states", "correction", "orbitals", "optimized"] and dm["optimized"].default is False
    iw = inspect.signature(abz.dos.integration_weights).parameters
    assert list(iw) == ["prob_or_cache", "E", "nstates", "kind", "correction", "fold", "optimized"] and iw["optimized"].default is False
    de = inspect.signature(abz.dos.density_matrix).parameters
    assert list(de) == ["prob_or_cache", "E", "nstates", "kind", "correction", "orbitals", "optimized"] and de["optimized"].default is False
    assert "negative" in abz.DeviceRule.ltm_node_weights_optimized.__doc__ and "negative" in abz.dos.integration_weights.__doc__


def test_node_weights_optimized_front_end_refusals():
    """the refusals the front end makes itself, before a device is asked for anything"""
    import autobzcore.jl_amd as abz
    c, first = case_coefficients(3)
    s = abz.FourierSeries(c, period=1.0, first=first, ndim=3)
    prob = abz.DOSProblem(s, 0.0, abz.load_bz(abz.FBZ(), np.eye(3)))
    for f in (abz.dos.integration_weights, abz.dos.density_matrix):
        with pytest.raises(ValueError, match="correction"):
            f(prob, E=0.3, correction=True, optimized=True)
        with pytest.raises(ValueError, match="correction"):
            f(prob, nstates=1.3, correction=True, optimized=True)
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    prob1 = abz.DOSProblem(h, 0.3, abz.load_bz(abz.FBZ(), [[2 * np.pi]]))
    for f in (abz.dos.integration_weights, abz.dos.density_matrix):
        with pytest.raises(NotImplementedError, match="d = 3"):
            f(prob1, E=0.3, optimized=True)

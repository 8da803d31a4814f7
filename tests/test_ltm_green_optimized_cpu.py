"""Green's functions of the optimized tetrahedron method, CPU side: the conditioning of the parity cases of the device test, what
the rule is for -- tr G(z) at a fixed grid --, the identities of the restatement (tests/goptltm_numpy.py) and the bindings of
abz_rule_ltm_green_optimized.  The device kernel is checked against the same restatement in test_gpu_ltm_green_optimized.py."""
import inspect
import os
import re

import numpy as np
import pytest

import gltm_numpy as gn
import goptltm_numpy as gon
import optltm_numpy as on
from test_ltm_optimized_cpu import GRIDS, SEEDS, case_coefficients, case_elements

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_eigenvalues(n, npt):
    import abz_oracle as orc
    import ltm_numpy as ln
    c, first = case_coefficients(n)
    return ln.grid_eigenvalues(orc.FourierSeries(c, period=1.0, first=first, ndim=3), npt)


def sources(eig, A):
    """label -> the restatement's `A` argument.  The energy rides as component 0 of the elements: A' = P e is the very product
    that "energy" takes, and the corner weights of a z are then formed once for all six components."""
    return {"trace": None, "energy and elements": np.concatenate([eig[None], A.reshape((A.shape[0],) + eig.shape)])}


# ---------------------------------------------------------------- 1. conditioning of the parity cases
@pytest.mark.parametrize("n", sorted(SEEDS))
@pytest.mark.parametrize("npt", GRIDS)
def test_cases_are_well_conditioned(n, npt):
    """e' from the f64 product against e' from a longdouble product rounded to f64, through the same closed forms: what the
    rounding of the 20-point product does to tr G and G_A at the z lists of the device test.  The bound is a tenth of the
    device test's, so that its 1e-9 is a statement about the kernel."""
    eig = case_eigenvalues(n, npt)
    A = case_elements(n, npt)
    for label, zs in gon.z_lists(eig).items():
        for src, arg in sources(eig, A).items():
            u = gon.green(eig, arg, zs)
            v = gon.green(eig, arg, zs, dtype=np.longdouble)
            assert np.all(np.isfinite(u.view(np.float64)))
            worst = float(np.abs(u - v).max()) / max(1.0, float(np.abs(v).max()))
            print(f"n = {n}, npt = {npt}, {label}, {src}: f64 against longdouble {worst:.2e} of the scale")
            assert worst <= 1e-10, (label, src, worst)


# ---------------------------------------------------------------- 2. what the rule is for
def test_trace_at_a_fixed_grid_converges_faster():
    """tr G(z) of e(k) = -2 sum_i cos 2 pi k_i + 0.5 cos 2 pi (k_1 + k_2) at z = (-1.3, 0.4, -4.0) + 0.2j, errors against the
    optimized restatement at npt = 48.  Condition: the optimized error at npt = 16 is at most a fifth of the plain error at 16."""
    zs = np.array([-1.3, 0.4, -4.0]) + 0.2j
    ref = gon.green(on.issue_band(48), None, zs)
    eig = on.issue_band(16)
    plain = np.abs(gon.green(eig, None, zs, optimized=False) - ref)
    opt = np.abs(gon.green(eig, None, zs) - ref)
    for z, p, o in zip(zs, plain, opt):
        print(f"tr G({z}) at npt = 16 against the optimized sum at 48: plain {p:.3e}, optimized {o:.3e}, ratio {p / o:.1f}")
    assert np.all(opt <= plain / 5.0)


# ---------------------------------------------------------------- 3. identities of the restatement
def test_restatement_identities():
    n, npt = 3, 5
    eig = case_eigenvalues(n, npt)
    zs = gon.z_lists(eig)["generic"]
    tr = gon.green(eig, None, zs)
    # sum_i W_i = J: A = 1 gives A' = 1 (the rows of P sum to one) and the trace
    ones = gon.green(eig, np.ones((1,) + eig.shape), zs)[:, 0]
    assert np.abs(ones - tr).max() <= 1e-12 * max(1.0, np.abs(tr).max())
    # sum_i x_i W_i = z J - 1 on the effective corners (the parity bound of the device test, which asks the same of the kernel)
    en = gon.green(eig, "energy", zs)[:, 0]
    print(f"A = 1 against the trace {np.abs(ones - tr).max():.2e}, energy against z tr G - n {np.abs(en - (zs * tr - n)).max():.2e}")
    assert np.abs(en - (zs * tr - n)).max() <= 1e-9 * max(1.0, np.abs(en).max())
    # the plain corner values through the same composition are the linear rule
    lin = gn.green_trace(eig, zs)
    assert np.abs(gon.green(eig, None, zs, optimized=False) - lin).max() <= 1e-13 * max(1.0, np.abs(lin).max())
    # and the optimized rule is another rule
    assert np.abs(tr - lin).max() > 1e-4


# ---------------------------------------------------------------- 4. bindings
def test_green_optimized_bindings():
    import autobzcore.jl_amd as abz
    L = abz._lib
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    assert re.search(r"^int abz_rule_ltm_green_optimized\(abz_rule\* r, int source, const double\* z /\* \[nz\]\[2\] \*/, int nz,\s+"
                     r"double\* out /\* \[nz\]\[ncomp\]\[2\] \*/\);", hdr, flags=re.M)
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_VERSION"] == 502 and defs["ABZ_K_COUNT"] == 8
    assert L.PROTOTYPES["abz_rule_ltm_green_optimized"] == L.PROTOTYPES["abz_rule_ltm_green_weighted"]
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert ":abz_rule_ltm_green_optimized" in jl and "function ltm_green_optimized(" in jl
    mk = open(os.path.join(ROOT, "autobzcore.jl_amd", "csrc", "Makefile")).read()
    assert "kernels_ltm_green_opt.o" in mk
    # the new keyword comes last and defaults to the linear rule
    assert list(inspect.signature(abz.DeviceRule.ltm_green_optimized).parameters) == ["self", "zs", "elements"]
    assert list(inspect.signature(abz.DeviceRule.ltm_green_optimized).parameters) == list(inspect.signature(abz.DeviceRule.ltm_green).parameters)
    for f in (abz.dos.green_trace, abz.dos.green_weighted):
        p = inspect.signature(f).parameters
        assert list(p) == ["prob_or_cache", "zs", "optimized"] and p["optimized"].default is False
    # the solve path with eta stays the linear rule's
    with pytest.raises(ValueError, match="eta"):
        abz.LTM(optimized=True, eta=0.1)
    # a null handle is refused before anything else is looked at
    assert L.lib().abz_rule_ltm_green_optimized(None, L.LTM_A_ONE, None, 1, None) == L.ERR_ARG
    assert b"null rule handle" in L.lib().abz_last_error()

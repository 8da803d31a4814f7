"""Without a GPU: the cases of tests/pivot_cases.py are what they claim to be -- well conditioned, returned accurately by
LAPACK's pivoting `inv`, destroyed by an elimination without pivoting -- and the C ABI of the pivoting mode is declared,
bound and exported."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pivot_cases as pc
import resolvent_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ALL = pc.all_cases()


@pytest.mark.parametrize("p", _ALL, ids=[pc.case_id(p) for p in _ALL])
def test_case_properties(p):
    case = pc.get(p)
    assert case.eta == 0.0 and case.sweep[case.one] == 0.0
    assert (np.diagonal(case.Hk, axis1=-2, axis2=-1) == 0.0).all()  # entry (0, 0) of z I - H(k) is z exactly
    assert case.cond <= 4.0, case.cond
    assert case.residual <= 1e-15  # (refined_inverse raises beyond its default tolerance: the reference converged)
    G = np.asarray(case.ref("gloc")).reshape(len(case.sweep), case.n, case.n)  # [s][column][row]
    for i, om in enumerate(case.sweep):
        unit = rr.EPS * case.amp[i]
        lap = rr.lapack_sum(case.Hk, case.w, complex(om, case.eta))
        e_lap = float(np.abs(lap.T.astype(np.clongdouble) - G[i]).max())
        un = pc.unpivoted_sum(case.Hk, case.w, complex(om, case.eta))
        print(f"{case.name} omega = {om:g}: LAPACK err / (eps A) {e_lap / unit:.3g}")
        assert e_lap <= rr.K_BOUND * unit
        if om == 0.0:
            assert not np.isfinite(un.view(np.float64)).all()
        if om == 1e-9:
            e_un = float(np.abs(un.T.astype(np.clongdouble) - G[i]).max())
            print(f"{case.name} omega = {om:g}: unpivoted err / (eps A) {e_un / unit:.3g}")
            assert e_un > 1e3 * rr.K_BOUND * unit


def test_paired_family_is_exactly_hermitian():
    for n in pc.PAIRED_BANDS:
        case = pc.paired_case(n)
        flip = case.c[tuple(slice(None, None, -1) for _ in range(case.d))]
        assert np.array_equal(case.c, np.conj(np.swapaxes(flip, -1, -2)))
    for fam in ("shift", "derangement"):
        case = pc.get((fam, 2, None, None))
        assert not np.allclose(case.Hk, np.conj(np.swapaxes(case.Hk, -1, -2)))


def test_derangements_have_no_fixed_point():
    for n in pc.NONHERM_BANDS:
        c = pc.get(("derangement", n, None, None)).c
        const = c[(1,) * (c.ndim - 2)]
        big = np.abs(const) > 0.5
        assert (big.sum(axis=0) == 1).all() and (big.sum(axis=1) == 1).all() and not big.diagonal().any()
        assert np.allclose(np.abs(const[big]), 1.0, atol=0.5)


# ---------------------------------------------------------------------------------------------------------------- the ABI
_SYMS = ("abz_series_set_pivoting", "abz_series_get_pivoting")


def test_pivoting_abi_declared_bound_and_exported():
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    declared = set(re.findall(r"^(?:const char\*|int) (abz_\w+)\(", hdr, flags=re.M))
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert (defs["ABZ_PIVOT_NONE"], defs["ABZ_PIVOT_PARTIAL"]) == (L.PIVOT_NONE, L.PIVOT_PARTIAL) == (0, 1)
    h = L.lib()
    for name in _SYMS:
        assert name in declared and name in L.PROTOTYPES
        assert hasattr(h, name)
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    for name in _SYMS:
        assert f"(:{name}, libabz)" in jl


def test_pivoting_null_series_is_an_argument_error():
    from autobzcore.jl_amd import _lib as L
    h = L.lib()
    m = C.c_int(7)
    assert h.abz_series_set_pivoting(None, L.PIVOT_PARTIAL) == L.ERR_ARG
    assert h.abz_series_get_pivoting(None, C.byref(m)) == L.ERR_ARG
    assert m.value == 7


def test_python_mirror_refuses_a_bad_mode():
    import autobzcore.jl_amd as abz
    for cls in (abz.DOSIntegrand, abz.TrGlocIntegrand, abz.GlocIntegrand):
        assert cls(pivoting="partial").pivoting == "partial" and cls().pivoting is None
        with pytest.raises(ValueError):
            cls(pivoting="complete")

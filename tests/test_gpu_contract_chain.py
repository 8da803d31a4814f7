"""contract_chain_kernel: variables 3 and 2 of a 3-D full grid contracted in one launch.

The fused launch must give the very sums of the per-level launches (ABZ_CHAIN_FUSED=0), bit for bit: rule exports
(H, eigenvalues), abz_rule_reduce values, slab rules and the store-free abz_ptr_sum.  Two cases are also checked
against the oracle, and the ABZ_K_CONTRACT launch count shows which path ran.
"""
import os

import numpy as np
import pytest

import abz_oracle as orc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


@pytest.fixture(scope="module")
def svo_c(abz):
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    return s.c, s.first


def _series(rng, dims, n, hermitian):
    c = rng.standard_normal(dims + (n, n)) + 1j * rng.standard_normal(dims + (n, n))
    first = tuple(-(m // 2) for m in dims)
    if hermitian:
        flip = c[::-1, ::-1, ::-1]
        c = 0.5 * (c + np.conj(np.swapaxes(flip, -1, -2)))
    return c, first


def _both(monkeypatch, fn):
    """fn() with the fused chain (the default), then with one launch per contraction level."""
    monkeypatch.delenv("ABZ_CHAIN_FUSED", raising=False)
    a = fn()
    monkeypatch.setenv("ABZ_CHAIN_FUSED", "0")
    try:
        b = fn()
    finally:
        monkeypatch.delenv("ABZ_CHAIN_FUSED")
    return a, b


def _rule_data(abz, c, first, npt, H=True, eig=True, omegas=None, kshard=None):
    """Export of a freshly built rule (and DOS sums when `omegas` is given); a new series each time, so no rule is cached."""
    L = abz._lib
    dev = abz.FourierSeries(c, period=1.0, first=first, ndim=3).device()
    dev.kshard, dev.allreduce = kshard, ((lambda a: a) if kshard else None)
    try:
        rule = dev.rule(npt, None, (L.WANT_H if H else 0) | (L.WANT_EIG if eig else 0))
        out = rule.export(x=False, w=False, H=H, eig=eig)
        if omegas is not None:
            out["dos"] = rule.reduce(L.F_DOS_EIG if eig else L.F_DOS, [0.1], omegas)
        rule.close()
    finally:
        dev.kshard, dev.allreduce = None, None
        dev.drop_rules()
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("npt", [37, 64, 96])
def test_svo_rule_bitwise(abz, svo_c, monkeypatch, npt):
    c, first = svo_c
    om = np.linspace(11.0, 14.0, 5)
    a, b = _both(monkeypatch, lambda: _rule_data(abz, c, first, npt, omegas=om))
    _assert_same(a, b)


def test_svo_150_eigenvalues_and_dos_bitwise(abz, svo_c, monkeypatch):
    """The benchmark's grid: eigenvalues and a 16-omega DOS sum only (host memory)."""
    c, first = svo_c
    om = np.linspace(10.0, 15.0, 16)
    a, b = _both(monkeypatch, lambda: _rule_data(abz, c, first, 150, H=False, omegas=om))
    _assert_same(a, b)


# dims = coefficients of variables 1, 2, 3 (M2 = dims[1], M3 = dims[2]); Hermitian cases have odd counts (packed rows
# for n <= 4), the others run on unpacked rows; n = 6 and 16 take the generic-n rule path (rows of 2 and 12 column blocks)
CASES = [
    ((5, 1, 7), 1, True, 23),
    ((3, 13, 1), 2, True, 20),
    ((7, 3, 15), 3, True, 17),
    ((5, 9, 11), 4, True, 24),
    ((3, 5, 7), 6, True, 13),
    ((3, 3, 5), 16, True, 7),
    ((3, 16, 5), 2, False, 19),
    ((4, 6, 16), 3, False, 11),
]


@pytest.mark.parametrize("dims,n,herm,npt", CASES)
def test_synthetic_rules_bitwise(abz, monkeypatch, dims, n, herm, npt):
    rng = np.random.default_rng(900 + 7 * n + sum(dims))
    c, first = _series(rng, dims, n, herm)
    a, b = _both(monkeypatch, lambda: _rule_data(abz, c, first, npt, eig=herm, omegas=np.linspace(-2, 2, 3)))
    _assert_same(a, b)


@pytest.mark.parametrize("dims,n,herm,npt", [((5, 9, 11), 4, True, 24), ((3, 16, 5), 2, False, 19)])
def test_against_the_oracle(abz, dims, n, herm, npt):
    """Fused chain (the default) against fourier_ptr at the tolerance of the existing rule tests."""
    rng = np.random.default_rng(950 + n)
    c, first = _series(rng, dims, n, herm)
    got = _rule_data(abz, c, first, npt, eig=False)["H"]
    vals = orc.fourier_ptr(orc.FourierSeries(c, period=1.0, first=first, ndim=3), npt)
    ref = np.transpose(vals, (2, 1, 0, 3, 4)).reshape(-1, n, n)  # column-major node order
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_slab_rules_bitwise_and_rows_of_the_full_rule(abz, monkeypatch):
    """k-sharded slabs of the outermost variable (abz_ptr_rule_build_slab): every slab is the same with either path, and
    the slabs' rows are the full rule's rows."""
    rng = np.random.default_rng(977)
    c, first = _series(rng, (5, 7, 9), 3, True)
    npt, W = 21, 4
    full = _rule_data(abz, c, first, npt)
    rows = []
    for r in range(W):
        a, b = _both(monkeypatch, lambda: _rule_data(abz, c, first, npt, kshard=(r, W)))
        _assert_same(a, b)
        rows.append(a)
    for k in ("H", "eig"):
        assert np.array_equal(np.concatenate([e[k] for e in rows]), full[k]), k


@pytest.mark.parametrize("n", [3, 6])
def test_store_free_sum_bitwise(abz, monkeypatch, n):
    L = abz._lib
    rng = np.random.default_rng(990 + n)
    c, first = _series(rng, (5, 7, 3), n, True)
    om = np.linspace(-1.5, 1.5, 6)

    def run():
        dev = abz.FourierSeries(c / 2, period=1.0, first=first, ndim=3).device()
        out = {f: dev.ptr_sum(40, f, [0.3], om) for f in (L.F_DOS, L.F_TRGLOC)}
        dev.drop_rules()
        return out

    a, b = _both(monkeypatch, run)
    _assert_same(a, b)


def test_one_contraction_launch_per_rebuild(abz, svo_c, monkeypatch):
    """The fused kernel ran: one ABZ_K_CONTRACT launch per rebuild by default, two with ABZ_CHAIN_FUSED=0."""
    L = abz._lib
    c, first = svo_c

    def launches():
        dev = abz.FourierSeries(c, period=1.0, first=first, ndim=3).device()
        rule = dev.rule(24, None, L.WANT_H | L.WANT_EIG)
        ctx = dev.ctx
        ctx.prof_enable(True, kernels=[L.K_CONTRACT])
        ctx.prof_reset()
        for _ in range(3):
            rule.rebuild()
        ctx.sync()
        _, nl = ctx.prof_read(L.K_CONTRACT)
        ctx.prof_enable(False)
        rule.close()
        dev.drop_rules()
        return nl

    fused, per_level = _both(monkeypatch, launches)
    assert (fused, per_level) == (3, 6)

"""Fused instance of eval_grid_kernel: the last contraction of a 3-D full grid inside the grid kernel, from LDS.

By default the chain stops at the level-2 sets and every wave of the grid kernel contracts its own lines; with
ABZ_EVAL_FUSED=0 contract_chain_kernel writes the level-1 sets and the plain grid kernel reads them.  Both run the same
fma sequences, so everything below is compared bit for bit: rule exports (H, eigenvalues) and a short abz_rule_reduce
DOS sum.  Two cases are also checked against the oracle, and the ABZ_K_EVAL_FUSED launch count shows which route ran (both
routes make one ABZ_K_CONTRACT and one ABZ_K_EVAL launch per rebuild, so those counts cannot tell them apart).
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
    """fn() with the fused grid kernel (the default), then with level-1 sets in memory."""
    monkeypatch.delenv("ABZ_EVAL_FUSED", raising=False)
    monkeypatch.delenv("ABZ_CHAIN_FUSED", raising=False)
    a = fn()
    monkeypatch.setenv("ABZ_EVAL_FUSED", "0")
    try:
        b = fn()
    finally:
        monkeypatch.delenv("ABZ_EVAL_FUSED")
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


@pytest.mark.parametrize("npt", [3, 24, 37])
def test_svo_rule_bitwise(abz, svo_c, monkeypatch, npt):
    """npt = 3: fewer lines per outermost index than waves in a block; 37: lines per index no multiple of 4.  KPL = 1."""
    c, first = svo_c
    om = np.linspace(11.0, 14.0, 5)
    a, b = _both(monkeypatch, lambda: _rule_data(abz, c, first, npt, omegas=om))
    _assert_same(a, b)


@pytest.mark.parametrize("npt,kshard", [(70, (5, 16)), (130, (7, 32)), (193, (9, 64)), (260, (3, 130))])
def test_svo_nodes_per_lane_on_slabs_bitwise(abz, svo_c, monkeypatch, npt, kshard):
    """70: two nodes per lane; 130: three, with idle tail lanes; 193: two, and two passes per line; 260: a phase table of
    more entries than a block has threads.  Slabs keep them small."""
    c, first = svo_c
    om = np.linspace(11.0, 14.0, 5)
    a, b = _both(monkeypatch, lambda: _rule_data(abz, c, first, npt, omegas=om, kshard=kshard))
    assert a["eig"].shape[0] > 0
    _assert_same(a, b)


def test_svo_150_eigenvalues_and_dos_bitwise(abz, svo_c, monkeypatch):
    """The benchmark's grid (the non-temporal store path): eigenvalues and a 16-omega DOS sum only (host memory)."""
    c, first = svo_c
    om = np.linspace(10.0, 15.0, 16)
    a, b = _both(monkeypatch, lambda: _rule_data(abz, c, first, 150, H=False, omegas=om))
    _assert_same(a, b)


# dims = coefficients of variables 1, 2, 3 (M2 = dims[1], M3 = dims[2]).  Hermitian cases have odd counts (packed rows),
# the others run on unpacked rows with even counts.  The level-2 set of (16, 16, 4) with 4 bands (16 x 16 x 16 numbers) exceeds the
# grid kernel's LDS: it takes the chain kernel on both arms.  (8, 12, 3) with 4 bands: two columns per lane and a level-2
# set of more than four numbers per thread of the block.
CASES = [
    ((5, 3, 7), 1, True, 23),
    ((3, 13, 5), 2, True, 20),
    ((7, 3, 15), 3, True, 17),
    ((5, 9, 11), 4, True, 24),
    ((4, 6, 8), 2, False, 19),
    ((4, 6, 16), 3, False, 11),
    ((5, 1, 7), 3, True, 21),
    ((3, 16, 5), 2, False, 19),
    ((5, 7, 1), 2, True, 18),
    ((16, 16, 4), 4, False, 9),
    ((8, 12, 3), 4, False, 10),
]


@pytest.mark.parametrize("dims,n,herm,npt", CASES)
def test_synthetic_rules_bitwise(abz, monkeypatch, dims, n, herm, npt):
    rng = np.random.default_rng(1900 + 7 * n + sum(dims))
    c, first = _series(rng, dims, n, herm)
    a, b = _both(monkeypatch, lambda: _rule_data(abz, c, first, npt, eig=herm, omegas=np.linspace(-2, 2, 3)))
    _assert_same(a, b)


@pytest.mark.parametrize("flavour", ["H", "eig", "reference"])
def test_rule_flavours_bitwise(abz, monkeypatch, flavour):
    """H only, eigenvalues only, and H with eigenvalues in the reference (full SMatrix) layout."""
    rng = np.random.default_rng(1931)
    c, first = _series(rng, (5, 7, 9), 3, True)
    if flavour == "reference":
        monkeypatch.setenv("ABZ_RULE_COMPACT", "0")
    kw = dict(H=flavour != "eig", eig=flavour != "H")
    a, b = _both(monkeypatch, lambda: _rule_data(abz, c, first, 22, omegas=np.linspace(-2, 2, 3), **kw))
    _assert_same(a, b)


def test_slab_rules_bitwise_and_rows_of_the_full_rule(abz, monkeypatch):
    rng = np.random.default_rng(1977)
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


def test_rebuild_after_update(abz, monkeypatch):
    """New coefficients reach the level-2 sets: a rebuilt rule holds the values of a rule built from them afresh."""
    L = abz._lib
    rng = np.random.default_rng(1990)
    c0, first = _series(rng, (5, 7, 9), 3, True)
    c1, _ = _series(rng, (5, 7, 9), 3, True)
    fresh = _rule_data(abz, c1, first, 20)

    def run():
        dev = abz.FourierSeries(c0, period=1.0, first=first, ndim=3).device()
        rule = dev.rule(20, None, L.WANT_H | L.WANT_EIG)
        dev.update(c1)
        rule.rebuild()
        out = rule.export(x=False, w=False, H=True, eig=True)
        rule.close()
        dev.drop_rules()
        return out

    a, b = _both(monkeypatch, run)
    _assert_same(a, b)
    _assert_same(a, fresh)


@pytest.mark.parametrize("dims,n,herm,npt", [((5, 9, 11), 4, True, 24), ((4, 6, 8), 2, False, 19)])
def test_against_the_oracle(abz, monkeypatch, dims, n, herm, npt):
    """The fused grid kernel (the default) against fourier_ptr at the tolerance of the existing rule tests."""
    monkeypatch.delenv("ABZ_EVAL_FUSED", raising=False)
    monkeypatch.delenv("ABZ_CHAIN_FUSED", raising=False)
    rng = np.random.default_rng(1950 + n)
    c, first = _series(rng, dims, n, herm)
    got = _rule_data(abz, c, first, npt, eig=False)["H"]
    vals = orc.fourier_ptr(orc.FourierSeries(c, period=1.0, first=first, ndim=3), npt)
    ref = np.transpose(vals, (2, 1, 0, 3, 4)).reshape(-1, n, n)  # column-major node order
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def _launches(abz, c, first, npt, want_eig=True, kshard=None):
    """(ABZ_K_CONTRACT, ABZ_K_EVAL, ABZ_K_EVAL_FUSED) launches of three rebuilds of a fresh rule."""
    L = abz._lib
    dev = abz.FourierSeries(c, period=1.0, first=first, ndim=3).device()
    dev.kshard, dev.allreduce = kshard, ((lambda a: a) if kshard else None)
    try:
        rule = dev.rule(npt, None, L.WANT_H | (L.WANT_EIG if want_eig else 0))
    finally:
        dev.kshard, dev.allreduce = None, None
    ctx = dev.ctx
    ids = [L.K_CONTRACT, L.K_EVAL, L.K_EVAL_FUSED]
    ctx.prof_enable(True, kernels=ids)
    ctx.prof_reset()
    for _ in range(3):
        rule.rebuild()
    ctx.sync()
    out = tuple(ctx.prof_read(k)[1] for k in ids)
    ctx.prof_enable(False)
    rule.close()
    dev.drop_rules()
    return out


def test_which_route_ran(abz, svo_c, monkeypatch):
    """By default the fused grid kernel runs behind one contraction launch; ABZ_EVAL_FUSED=0 and a level-2 set beyond the
    grid kernel's LDS take the chain kernel and the plain instance; ABZ_CHAIN_FUSED=0 the two per-level launches."""
    c, first = svo_c
    fused, chain = _both(monkeypatch, lambda: _launches(abz, c, first, 24))
    assert fused == (3, 3, 3)
    assert chain == (3, 3, 0)
    monkeypatch.setenv("ABZ_CHAIN_FUSED", "0")
    assert _launches(abz, c, first, 24) == (6, 3, 0)
    monkeypatch.delenv("ABZ_CHAIN_FUSED")
    rng = np.random.default_rng(1900 + 7 * 4 + 36)
    big, bfirst = _series(rng, (16, 16, 4), 4, False)
    assert _launches(abz, big, bfirst, 9, want_eig=False) == (3, 3, 0)
    small, sfirst = _series(rng, (4, 6, 8), 2, False)
    assert _launches(abz, small, sfirst, 19, want_eig=False) == (3, 3, 3)


def test_size_rule_of_the_reference_layout(abz, svo_c, monkeypatch):
    """Full-matrix rules of a Hermitian series keep the chain kernel beyond 64 points (slabs of two planes here); the
    upper-triangle layout and smaller grids take the fused grid kernel."""
    c, first = svo_c
    monkeypatch.delenv("ABZ_EVAL_FUSED", raising=False)
    monkeypatch.delenv("ABZ_CHAIN_FUSED", raising=False)
    assert _launches(abz, c, first, 130, kshard=(7, 65)) == (3, 3, 3)
    monkeypatch.setenv("ABZ_RULE_COMPACT", "0")
    assert _launches(abz, c, first, 130, kshard=(7, 65)) == (3, 3, 0)
    assert _launches(abz, c, first, 64, kshard=(7, 32)) == (3, 3, 3)

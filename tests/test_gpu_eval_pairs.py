"""Pair mapping of the fused grid kernel: one grid line per half-wave (eval_grid_kernel, mapping fused_pairs).

Per node the pair mapping runs the arithmetic of the 64-lane mapping on the same operands; only the lane a node sits in
changes.  So three arms are compared bit for bit: ABZ_EVAL_PAIRS=2 (pairs wherever the kernel supports them: small grids
tie in the launcher's lane-round count and would keep the 64-lane mapping), ABZ_EVAL_PAIRS=0 (the 64-lane mapping
everywhere) and ABZ_EVAL_FUSED=0 (level-1 sets in memory, the plain grid kernel).  Compared are rule exports (H,
eigenvalues) and a short abz_rule_reduce DOS sum; one case is also checked against the oracle.

Which mapping ran cannot be told from the existing counters: ABZ_K_EVAL_FUSED counts the launches of the fused instance
in either mapping, and both make one ABZ_K_CONTRACT and one ABZ_K_EVAL launch per rebuild.  The route test shows that the
fused instance ran in both arms; that the arms differ rests on the forced switch.
"""
import os

import numpy as np
import pytest

import abz_oracle as orc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ARMS = (("pairs", {"ABZ_EVAL_PAIRS": "2"}), ("lines", {"ABZ_EVAL_PAIRS": "0"}), ("unfused", {"ABZ_EVAL_FUSED": "0"}))


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


def _arms(monkeypatch, fn):
    """{arm: fn()} with forced pairs, with the 64-lane mapping, and with level-1 sets in memory."""
    out = {}
    for name, env in ARMS:
        for k in ("ABZ_EVAL_PAIRS", "ABZ_EVAL_FUSED", "ABZ_CHAIN_FUSED"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            out[name] = fn()
        finally:
            for k in env:
                monkeypatch.delenv(k)
    return out


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
        assert a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k]), k


def _assert_arms_same(r):
    _assert_same(r["pairs"], r["lines"])
    _assert_same(r["pairs"], r["unfused"])


@pytest.mark.parametrize("npt", [5, 33, 37])
def test_svo_rule_bitwise(abz, svo_c, monkeypatch, npt):
    """5: odd, fewer pairs than waves in a block, the last pair a single line; 33: a second round that holds one column;
    37: odd, pairs per outermost index no multiple of 4."""
    c, first = svo_c
    om = np.linspace(11.0, 14.0, 5)
    r = _arms(monkeypatch, lambda: _rule_data(abz, c, first, npt, omegas=om))
    assert r["pairs"]["eig"].shape[0] == npt**3
    _assert_arms_same(r)


@pytest.mark.parametrize("npt,kshard", [(70, (5, 16)), (150, (7, 75)), (193, (9, 64)), (260, (3, 130)), (37, (36, 37))])
def test_svo_rounds_on_slabs_bitwise(abz, svo_c, monkeypatch, npt, kshard):
    """70: three rounds in one pass; 150 on two planes: the benchmark's instance, a pass of three rounds and one of two,
    10 filler columns; 193: seven rounds, three passes; 260: a phase table of more entries than a block has threads;
    37 on (36, 37): a slab of one plane.  Slabs keep them small."""
    c, first = svo_c
    om = np.linspace(11.0, 14.0, 5)
    r = _arms(monkeypatch, lambda: _rule_data(abz, c, first, npt, omegas=om, kshard=kshard))
    assert r["pairs"]["eig"].shape[0] > 0 and r["pairs"]["eig"].shape[0] % (npt * npt) == 0
    if npt == 37:
        assert r["pairs"]["eig"].shape[0] == npt * npt
    _assert_arms_same(r)


def test_svo_150_eigenvalues_and_dos_bitwise(abz, svo_c, monkeypatch):
    """The benchmark's grid (the non-temporal store path): the full 150^3 H + eigenvalue rule on the device; compared are
    the eigenvalue export and a 16-omega F_DOS sum, which reads the H planes (H is not exported: host memory)."""
    c, first = svo_c
    L = abz._lib
    om = np.linspace(10.0, 15.0, 16)

    def run():
        dev = abz.FourierSeries(c, period=1.0, first=first, ndim=3).device()
        try:
            rule = dev.rule(150, None, L.WANT_H | L.WANT_EIG)
            out = rule.export(x=False, w=False, H=False, eig=True)
            out["dos"] = rule.reduce(L.F_DOS, [0.1], om)
            rule.close()
        finally:
            dev.drop_rules()
        return out

    _assert_arms_same(_arms(monkeypatch, run))


# dims = coefficients of variables 1, 2, 3 (M2 = dims[1]).  Hermitian cases have odd counts (packed rows), the others run
# on unpacked rows with even counts.
CASES = [
    ((5, 3, 7), 1, True, 23),
    ((3, 13, 5), 2, True, 20),
    ((5, 9, 11), 4, True, 24),
    ((4, 6, 8), 2, False, 19),
    ((4, 6, 16), 3, False, 17),
    ((5, 1, 7), 3, True, 21),
]


@pytest.mark.parametrize("dims,n,herm,npt", CASES)
def test_synthetic_rules_bitwise(abz, monkeypatch, dims, n, herm, npt):
    rng = np.random.default_rng(2900 + 7 * n + sum(dims))
    c, first = _series(rng, dims, n, herm)
    r = _arms(monkeypatch, lambda: _rule_data(abz, c, first, npt, eig=herm, omegas=np.linspace(-2, 2, 3)))
    _assert_arms_same(r)


@pytest.mark.parametrize("flavour", ["H", "eig", "reference"])
def test_rule_flavours_bitwise(abz, monkeypatch, flavour):
    """H only, eigenvalues only, and H with eigenvalues in the reference (full SMatrix) layout: Hermitian, unpacked planes."""
    rng = np.random.default_rng(2931)
    c, first = _series(rng, (5, 7, 9), 3, True)
    if flavour == "reference":
        monkeypatch.setenv("ABZ_RULE_COMPACT", "0")
    kw = dict(H=flavour != "eig", eig=flavour != "H")
    r = _arms(monkeypatch, lambda: _rule_data(abz, c, first, 22, omegas=np.linspace(-2, 2, 3), **kw))
    _assert_arms_same(r)


def test_rebuild_after_update(abz, monkeypatch):
    """New coefficients reach both lines of every pair: the rebuilt rule holds the values of a rule built from them afresh."""
    L = abz._lib
    rng = np.random.default_rng(2990)
    c0, first = _series(rng, (5, 7, 9), 3, True)
    c1, _ = _series(rng, (5, 7, 9), 3, True)
    monkeypatch.setenv("ABZ_EVAL_PAIRS", "0")
    fresh = _rule_data(abz, c1, first, 21)
    monkeypatch.setenv("ABZ_EVAL_PAIRS", "2")
    dev = abz.FourierSeries(c0, period=1.0, first=first, ndim=3).device()
    rule = dev.rule(21, None, L.WANT_H | L.WANT_EIG)
    stale = rule.export(x=False, w=False, H=True, eig=True)
    dev.update(c1)
    rule.rebuild()
    out = rule.export(x=False, w=False, H=True, eig=True)
    rule.close()
    dev.drop_rules()
    assert not np.array_equal(stale["H"], out["H"])
    _assert_same(out, fresh)
    _assert_same(out, _rule_data(abz, c1, first, 21))


def test_against_the_oracle(abz, monkeypatch):
    """Forced pairs against fourier_ptr at the tolerance of the existing rule tests."""
    monkeypatch.setenv("ABZ_EVAL_PAIRS", "2")
    monkeypatch.delenv("ABZ_EVAL_FUSED", raising=False)
    monkeypatch.delenv("ABZ_CHAIN_FUSED", raising=False)
    dims, n, npt = (5, 9, 11), 4, 24
    rng = np.random.default_rng(2954)
    c, first = _series(rng, dims, n, True)
    got = _rule_data(abz, c, first, npt, eig=False)["H"]
    vals = orc.fourier_ptr(orc.FourierSeries(c, period=1.0, first=first, ndim=3), npt)
    ref = np.transpose(vals, (2, 1, 0, 3, 4)).reshape(-1, n, n)  # column-major node order
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def _launches(abz, c, first, npt):
    """(ABZ_K_CONTRACT, ABZ_K_EVAL, ABZ_K_EVAL_FUSED) launches of three rebuilds of a fresh rule."""
    L = abz._lib
    dev = abz.FourierSeries(c, period=1.0, first=first, ndim=3).device()
    rule = dev.rule(npt, None, L.WANT_H | L.WANT_EIG)
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
    """The fused instance runs in both mappings, behind one contraction launch and as one eval launch per rebuild; the
    counters do not tell the mappings apart (module docstring)."""
    c, first = svo_c
    r = _arms(monkeypatch, lambda: _launches(abz, c, first, 24))
    assert r["pairs"] == (3, 3, 3)
    assert r["lines"] == (3, 3, 3)
    assert r["unfused"] == (3, 3, 0)

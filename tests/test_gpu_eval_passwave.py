"""One pass of a line pair per wave in the fused pair mapping (eval_grid_kernel, mapping fused_passwave, ABZ_EVAL_PASSWAVE, DESIGN section 9
item 1).

The instance changes which wave evaluates which nodes and nothing of the arithmetic per node, so its rules are compared bit for
bit with the three other routes: a pair per wave (ABZ_EVAL_PASSWAVE=0), one grid line per wave (ABZ_EVAL_PAIRS=0) and level-1
sets in memory (ABZ_EVAL_FUSED=0).  Compared are rule exports (H, eigenvalues) and a 3-value DOS sum.  The route exists where a
pair takes 2 or 4 passes; with three rounds per pass (two with 4 bands) the grids below are the smallest that reach each
instance:

    npt  bands  rounds per pass
     97  1 2 3  3 + 1   last pass of one round; odd npt: the last pair has one line
    128  3      3 + 1   no padding columns
    129  3      3 + 2   the instance of the 150-point benchmark
     70  4      2 + 1   passes of two rounds

With real Hermitian coefficients the launch is mirrored (every arm with the mirror on: all routes mirror the same member of each
{k, -k} pair); 129 / 3 bands and 70 / 4 bands run again with a complex Hermitian series, which is not.  ABZ_K_EVAL_PASSWAVE
counts the launches of the instance, so the tests can tell that it ran.  The pair mapping is forced with ABZ_EVAL_PAIRS=2 in both
of its arms: at 97 and 128 points the launcher's lane-round count ties and would keep the 64-lane mapping.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SWITCHES = ("ABZ_EVAL_PASSWAVE", "ABZ_EVAL_MIRROR", "ABZ_EVAL_PAIRS", "ABZ_EVAL_FUSED", "ABZ_CHAIN_FUSED")
ARMS = {
    "passwave": {"ABZ_EVAL_MIRROR": "1", "ABZ_EVAL_PAIRS": "2", "ABZ_EVAL_PASSWAVE": "2"},
    "pairs": {"ABZ_EVAL_MIRROR": "1", "ABZ_EVAL_PAIRS": "2", "ABZ_EVAL_PASSWAVE": "0"},
    "lines": {"ABZ_EVAL_MIRROR": "1", "ABZ_EVAL_PAIRS": "0"},
    "unfused": {"ABZ_EVAL_MIRROR": "1", "ABZ_EVAL_FUSED": "0"},
}

DIMS = (3, 5, 7)  # coefficients of variables 1, 2, 3
# (npt, bands, real coefficients)
CASES = [(97, 1, True), (97, 2, True), (97, 3, True), (128, 3, True), (129, 3, True), (70, 4, True), (129, 3, False), (70, 4, False)]
IDS = [f"{npt}-{n}-{'real' if real else 'complex'}" for npt, n, real in CASES]


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def _hermitian(seed, dims, n, real):
    """Coefficients with c(-R) = c(R)^H; real: real ones, c(-R) = c(R)^T."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(dims + (n, n)) + (0.0 if real else 1j) * rng.standard_normal(dims + (n, n))
    c = 0.5 * (c + np.conj(np.swapaxes(c[::-1, ::-1, ::-1], -1, -2)))
    return c.astype(np.complex128), tuple(-(m // 2) for m in dims)


def _with_env(monkeypatch, env, fn):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return fn()
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _rule_data(abz, c, first, npt, omegas):
    """Export of a freshly built rule and a short DOS sum; a new series each time, so no rule is cached."""
    L = abz._lib
    dev = abz.FourierSeries(c, period=1.0, first=first, ndim=3).device()
    try:
        rule = dev.rule(npt, None, L.WANT_H | L.WANT_EIG)
        out = rule.export(x=False, w=False, H=True, eig=True)
        out["dos"] = rule.reduce(L.F_DOS_EIG, [0.1], omegas)
        rule.close()
    finally:
        dev.drop_rules()
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k], b[k]), (what, k)


def _launches(abz, c, first, npt):
    """(ABZ_K_CONTRACT, ABZ_K_EVAL, ABZ_K_EVAL_FUSED, ABZ_K_EVAL_PASSWAVE) launches of three rebuilds of a fresh rule."""
    L = abz._lib
    dev = abz.FourierSeries(c, period=1.0, first=first, ndim=3).device()
    try:
        rule = dev.rule(npt, None, L.WANT_H | L.WANT_EIG)
        ctx = dev.ctx
        ids = [L.K_CONTRACT, L.K_EVAL, L.K_EVAL_FUSED, L.K_EVAL_PASSWAVE]
        ctx.prof_enable(True, kernels=ids)
        ctx.prof_reset()
        for _ in range(3):
            rule.rebuild()
        ctx.sync()
        out = tuple(ctx.prof_read(k)[1] for k in ids)
        ctx.prof_enable(False)
        rule.close()
    finally:
        dev.drop_rules()
    return out


@pytest.mark.parametrize("npt,n,real", CASES, ids=IDS)
def test_same_rule_on_every_route(abz, monkeypatch, npt, n, real):
    c, first = _hermitian(5200 + n, DIMS, n, real)
    om = np.linspace(-2.0, 2.0, 3)
    got = _with_env(monkeypatch, ARMS["passwave"], lambda: _rule_data(abz, c, first, npt, om))
    assert got["eig"].shape[0] == npt**3 and np.isfinite(got["eig"]).all() and np.isfinite(got["dos"]).all()
    if real:  # mirrored: the planes k3 > npt / 2 hold conj H(-k), the registers of -k
        g = got["H"].reshape((npt, npt, npt) + got["H"].shape[1:])
        m = np.roll(g[::-1, ::-1, ::-1], 1, axis=(0, 1, 2))
        assert np.array_equal(g[npt // 2 + 1:], np.conj(m[npt // 2 + 1:]))
    for arm in ("pairs", "lines", "unfused"):
        other = _with_env(monkeypatch, ARMS[arm], lambda: _rule_data(abz, c, first, npt, om))
        _assert_same(got, other, arm)


def test_svo_24_points_keeps_the_pair_instance(abz, monkeypatch):
    """One round per pair: the route does not exist there, the switch at 2 changes nothing."""
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    om = np.linspace(11.0, 14.0, 3)
    got = _with_env(monkeypatch, ARMS["passwave"], lambda: _rule_data(abz, s.c, s.first, 24, om))
    for arm in ("pairs", "lines", "unfused"):
        _assert_same(got, _with_env(monkeypatch, ARMS[arm], lambda: _rule_data(abz, s.c, s.first, 24, om)), arm)
    assert _with_env(monkeypatch, ARMS["passwave"], lambda: _launches(abz, s.c, s.first, 24)) == (3, 3, 3, 0)


@pytest.mark.parametrize("npt,n,real", CASES, ids=IDS)
def test_no_unwritten_memory(abz, monkeypatch, npt, n, real):
    """The value block filled with NaN before a rebuild holds none after it: every column of every tile is written, the
    padding columns and both members of every {k, -k} pair included (the check of test_gpu_eval_mirror.py)."""
    L = abz._lib
    c, first = _hermitian(5200 + n, DIMS, n, real)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in ARMS["passwave"].items():
        monkeypatch.setenv(k, v)
    dev = abz.FourierSeries(c, period=1.0, first=first, ndim=3).device()
    try:
        rule = dev.rule(npt, None, L.WANT_H | L.WANT_EIG)
        base, nbytes = rule.values_ptr()
        assert base and nbytes > 0 and nbytes % 8 == 0
        dev.ctx.sync()
        memcpy = L.lib().hipMemcpy  # (the HIP runtime the library is linked against)
        memcpy.restype, memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        buf = np.full(nbytes // 8, np.nan)
        assert memcpy(base, buf.ctypes.data, nbytes, 1) == 0  # hipMemcpyHostToDevice
        ctx = dev.ctx
        ctx.prof_enable(True, kernels=[L.K_EVAL_PASSWAVE])
        ctx.prof_reset()
        rule.rebuild()
        ctx.sync()
        ran = ctx.prof_read(L.K_EVAL_PASSWAVE)[1]
        ctx.prof_enable(False)
        assert ran == 1
        assert memcpy(buf.ctypes.data, base, nbytes, 2) == 0  # hipMemcpyDeviceToHost
        assert not np.isnan(buf).any(), int(np.isnan(buf).sum())
        rule.close()
    finally:
        dev.drop_rules()


@pytest.mark.parametrize("real", [True, False])
def test_which_route_ran(abz, monkeypatch, real):
    """One contraction launch and one fused eval launch per rebuild on every arm; the new counter tells the instance."""
    c, first = _hermitian(5201, DIMS, 1, real)
    for arm, want in (("passwave", (3, 3, 3, 3)), ("pairs", (3, 3, 3, 0)), ("lines", (3, 3, 3, 0)), ("unfused", (3, 3, 0, 0))):
        assert _with_env(monkeypatch, ARMS[arm], lambda: _launches(abz, c, first, 97)) == want, arm


def test_default_selection(abz, monkeypatch):
    """No switch set: the instance runs where the launcher takes pairs by itself and a pair has two passes (129 points), not
    where it keeps one line per wave (128 points: the lane-round counts tie)."""
    c, first = _hermitian(5201, DIMS, 1, True)
    assert _with_env(monkeypatch, {}, lambda: _launches(abz, c, first, 129)) == (3, 3, 3, 3)
    assert _with_env(monkeypatch, {}, lambda: _launches(abz, c, first, 128)) == (3, 3, 3, 0)


def test_three_passes_keep_the_pair_instance(abz, monkeypatch):
    """193 points, one band: seven rounds in three passes, which do not divide a block's four waves."""
    c, first = _hermitian(5201, DIMS, 1, True)
    assert _with_env(monkeypatch, ARMS["passwave"], lambda: _launches(abz, c, first, 193)) == (3, 3, 3, 0)


def test_four_passes(abz, monkeypatch):
    """193 points with 4 bands: seven rounds in passes of two, 2 + 2 + 2 + 1, one pair per block.  Eigenvalues only (the rule
    with H would be 1.2 GB): the same on every route, every column written, and the instance ran."""
    L = abz._lib
    npt, n = 193, 4
    c, first = _hermitian(5204, DIMS, n, True)

    def eig_of_a_rebuild():
        dev = abz.FourierSeries(c, period=1.0, first=first, ndim=3).device()
        try:
            rule = dev.rule(npt, None, L.WANT_EIG)
            base, nbytes = rule.values_ptr()
            dev.ctx.sync()
            memcpy = L.lib().hipMemcpy
            memcpy.restype, memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            buf = np.full(nbytes // 8, np.nan)
            assert memcpy(base, buf.ctypes.data, nbytes, 1) == 0  # hipMemcpyHostToDevice
            ctx = dev.ctx
            ctx.prof_enable(True, kernels=[L.K_EVAL_FUSED, L.K_EVAL_PASSWAVE])
            ctx.prof_reset()
            rule.rebuild()
            ctx.sync()
            ran = (ctx.prof_read(L.K_EVAL_FUSED)[1], ctx.prof_read(L.K_EVAL_PASSWAVE)[1])
            ctx.prof_enable(False)
            assert memcpy(buf.ctypes.data, base, nbytes, 2) == 0  # hipMemcpyDeviceToHost
            assert not np.isnan(buf).any(), int(np.isnan(buf).sum())
            eig = rule.export(x=False, w=False, H=False, eig=True)["eig"]
            rule.close()
        finally:
            dev.drop_rules()
        return eig, ran

    got, ran = _with_env(monkeypatch, ARMS["passwave"], eig_of_a_rebuild)
    assert ran == (1, 1) and got.shape == (npt**3, n)
    for arm in ("pairs", "lines"):
        other, ran = _with_env(monkeypatch, ARMS[arm], eig_of_a_rebuild)
        assert ran == (1, 0), arm
        assert np.array_equal(got, other), arm


def test_rebuild_after_update(abz, monkeypatch):
    """A second rebuild() after update() with changed coefficients equals a fresh build of them."""
    L = abz._lib
    npt, n = 97, 2
    c0, first = _hermitian(5300, DIMS, n, True)
    c1, _ = _hermitian(5301, DIMS, n, True)
    om = np.linspace(-2.0, 2.0, 3)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in ARMS["passwave"].items():
        monkeypatch.setenv(k, v)
    fresh = [_rule_data(abz, c, first, npt, om) for c in (c0, c1)]
    assert not np.array_equal(fresh[0]["eig"], fresh[1]["eig"])
    dev = abz.FourierSeries(c0, period=1.0, first=first, ndim=3).device()
    try:
        rule = dev.rule(npt, None, L.WANT_H | L.WANT_EIG)
        for k in ("H", "eig"):
            assert np.array_equal(rule.export(x=False, w=False, H=True, eig=True)[k], fresh[0][k]), k
        dev.update(c1)
        rule.rebuild()
        for k in ("H", "eig"):
            assert np.array_equal(rule.export(x=False, w=False, H=True, eig=True)[k], fresh[1][k]), k
        rule.close()
    finally:
        dev.drop_rules()

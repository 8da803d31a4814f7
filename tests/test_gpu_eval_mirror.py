"""Mirrored rebuild of 3-D full-grid rules of a real Hermitian series (ABZ_EVAL_MIRROR).

For real coefficients with c(-R) = c(R)^T, H(-k) = conj H(k) entry by entry.  The grid kernels then evaluate the planes
k3 <= npt/2 only and store every node of a plane that is not its own mirror image a second time, conjugated, at -k.  So

* on the planes k3 <= npt/2 the rule is the switched-off build's bit for bit,
* elsewhere it holds conj H(-k) and the eigenvalues of -k bit for bit, which differ from what the switched-off build computes
  there by rounding only: the bound is the one tests/test_gpu_eval_pairs.py::test_against_the_oracle grants against the oracle,
* every route (pair mapping, 64-lane mapping, level-1 sets in memory) mirrors the same member of each {k, -k} pair,
* no column of the value block stays unwritten, padding included,
* anything else -- one imaginary part of 1e-300, a real series that is not Hermitian, a slab -- takes the route of
  ABZ_EVAL_MIRROR=0 bit for bit.

Node order of the exports: k = i1 + npt (i2 + npt i3); reshaped to [i3, i2, i1, ...] below.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SWITCHES = ("ABZ_EVAL_MIRROR", "ABZ_EVAL_PAIRS", "ABZ_EVAL_FUSED", "ABZ_CHAIN_FUSED")
ARMS = {
    "on": {"ABZ_EVAL_MIRROR": "1"},
    "off": {"ABZ_EVAL_MIRROR": "0"},
    "pairs": {"ABZ_EVAL_MIRROR": "1", "ABZ_EVAL_PAIRS": "2"},
    "lines": {"ABZ_EVAL_MIRROR": "1", "ABZ_EVAL_PAIRS": "0"},
    "unfused": {"ABZ_EVAL_MIRROR": "1", "ABZ_EVAL_FUSED": "0"},
}
RTOL = 1e-12  # tests/test_gpu_eval_pairs.py::test_against_the_oracle: |got - ref| <= 1e-12 max |ref|

DIMS = (3, 5, 7)  # coefficients of variables 1, 2, 3
GRIDS = (5, 6, 33, 64, 70, 75)
BANDS = (1, 2, 3, 4)
CASES = [(npt, n) for npt in GRIDS for n in BANDS] + [(24, "svo")]


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def _real_hermitian(rng, dims, n):
    """Real coefficients with c(-R) = c(R)^T."""
    c = rng.standard_normal(dims + (n, n))
    c = 0.5 * (c + np.swapaxes(c[::-1, ::-1, ::-1], -1, -2))
    return c.astype(np.complex128), tuple(-(m // 2) for m in dims)


_series_cache = {}


def _case_series(abz, n):
    if n not in _series_cache:
        if n == "svo":
            s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
            _series_cache[n] = (s.c, s.first)
        else:
            _series_cache[n] = _real_hermitian(np.random.default_rng(4100 + n), DIMS, n)
    return _series_cache[n]


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


_arm_cache = {}


def _arm(abz, monkeypatch, npt, n, arm):
    """The rule of case (npt, n) built in `arm`, with a short DOS sum; built once per module."""
    key = (npt, n, arm)
    if key not in _arm_cache:
        c, first = _case_series(abz, n)
        om = np.linspace(11.0, 14.0, 3) if n == "svo" else np.linspace(-2.0, 2.0, 3)
        _arm_cache[key] = _with_env(monkeypatch, ARMS[arm], lambda: _rule_data(abz, c, first, npt, omegas=om))
    return _arm_cache[key]


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k]), k


def _grid(a, npt):
    return a.reshape((npt, npt, npt) + a.shape[1:])


def _at_minus_k(g):
    """g[i3, i2, i1] -> g[-i3, -i2, -i1] (indices modulo npt)."""
    return np.roll(g[::-1, ::-1, ::-1], 1, axis=(0, 1, 2))


@pytest.mark.parametrize("npt,n", CASES)
def test_mirror_against_switched_off(abz, monkeypatch, npt, n):
    on, off = _arm(abz, monkeypatch, npt, n, "on"), _arm(abz, monkeypatch, npt, n, "off")
    half = npt // 2
    for key in ("H", "eig"):
        g_on, g_off = _grid(on[key], npt), _grid(off[key], npt)
        assert g_on.shape == g_off.shape
        # the evaluated planes: today's values
        assert np.array_equal(g_on[: half + 1], g_off[: half + 1]), key
        # the other planes: the registers of -k
        m = _at_minus_k(g_on)
        assert np.array_equal(g_on[half + 1:], np.conj(m[half + 1:])), key
        # ... which are what the switched-off build computes there, up to rounding
        err = np.abs(g_on[half + 1:] - g_off[half + 1:]).max() if half + 1 < npt else 0.0
        print(f"npt {npt} n {n} {key}: max |mirrored - evaluated| = {err:.3e}, scale {np.abs(g_off).max():.3e}")
        assert err <= RTOL * np.abs(g_off).max(), key


@pytest.mark.parametrize("npt,n", CASES)
def test_routes_mirror_alike(abz, monkeypatch, npt, n):
    """Pair mapping, 64-lane mapping and level-1 sets in memory take the same member of every {k, -k} pair."""
    on = _arm(abz, monkeypatch, npt, n, "on")
    for arm in ("pairs", "lines", "unfused"):
        _assert_same(on, _arm(abz, monkeypatch, npt, n, arm))


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


def test_launches_per_rebuild(abz, monkeypatch):
    """One contraction launch and one eval launch per rebuild, as in test_gpu_eval_pairs.py::test_which_route_ran."""
    c, first = _case_series(abz, "svo")
    for arm, want in (("on", (3, 3, 3)), ("pairs", (3, 3, 3)), ("lines", (3, 3, 3)), ("unfused", (3, 3, 0)), ("off", (3, 3, 3))):
        assert _with_env(monkeypatch, ARMS[arm], lambda: _launches(abz, c, first, 24)) == want, arm


def _hip_memcpy(abz):
    memcpy = abz._lib.lib().hipMemcpy  # (the HIP runtime the library is linked against)
    memcpy.restype, memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return memcpy


@pytest.mark.parametrize("want", ["H", "eig", "both"])
@pytest.mark.parametrize("layout", ["compact", "reference"])
@pytest.mark.parametrize("npt", [6, 33, 70])
def test_no_unwritten_memory(abz, monkeypatch, npt, layout, want):
    """The value block filled with NaN before a rebuild holds none after it: every column of every tile is written, the
    padding columns and both members of every {k, -k} pair included.  70 points in the reference layout is the plain grid
    kernel, 70 compact the pair mapping."""
    L = abz._lib
    c, first = _case_series(abz, 3)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ABZ_EVAL_MIRROR", "1")
    if layout == "reference":
        monkeypatch.setenv("ABZ_RULE_COMPACT", "0")
    dev = abz.FourierSeries(c, period=1.0, first=first, ndim=3).device()
    try:
        rule = dev.rule(npt, None, {"H": L.WANT_H, "eig": L.WANT_EIG, "both": L.WANT_H | L.WANT_EIG}[want])
        base, nbytes = rule.values_ptr()
        assert base and nbytes > 0 and nbytes % 8 == 0
        dev.ctx.sync()
        memcpy = _hip_memcpy(abz)
        buf = np.full(nbytes // 8, np.nan)
        assert memcpy(base, buf.ctypes.data, nbytes, 1) == 0  # hipMemcpyHostToDevice
        rule.rebuild()
        dev.ctx.sync()
        assert memcpy(buf.ctypes.data, base, nbytes, 2) == 0  # hipMemcpyDeviceToHost
        assert not np.isnan(buf).any(), int(np.isnan(buf).sum())
        rule.close()
    finally:
        dev.drop_rules()


def _on_and_off(abz, monkeypatch, c, first, npt, **kw):
    return (_with_env(monkeypatch, ARMS["on"], lambda: _rule_data(abz, c, first, npt, **kw)),
            _with_env(monkeypatch, ARMS["off"], lambda: _rule_data(abz, c, first, npt, **kw)))


@pytest.mark.parametrize("npt", [6, 33, 70])
def test_one_imaginary_part_switches_the_route_off(abz, monkeypatch, npt):
    """One coefficient pair with an imaginary part of 1e-300, still Hermitian: the values of ABZ_EVAL_MIRROR=0 bit for bit."""
    c, first = _case_series(abz, 3)
    c = c.copy()
    c[0, 1, 2, 0, 1] += 1e-300j
    c[-1, -2, -3, 1, 0] -= 1e-300j
    assert np.array_equal(c, np.conj(np.swapaxes(c[::-1, ::-1, ::-1], -1, -2))) and np.abs(c.imag).max() == 1e-300
    on, off = _on_and_off(abz, monkeypatch, c, first, npt)
    _assert_same(on, off)


@pytest.mark.parametrize("npt", [6, 33, 70])
def test_real_series_that_is_not_hermitian(abz, monkeypatch, npt):
    rng = np.random.default_rng(4177)
    c = rng.standard_normal(DIMS + (3, 3)).astype(np.complex128)
    first = tuple(-(m // 2) for m in DIMS)
    on, off = _on_and_off(abz, monkeypatch, c, first, npt, eig=False)
    _assert_same(on, off)


@pytest.mark.parametrize("kshard", [(0, 2), (1, 2)])
@pytest.mark.parametrize("npt", [6, 33, 70])
def test_slabs_keep_todays_route(abz, monkeypatch, npt, kshard):
    """A slab's mirror planes belong to another rank: each half of the grid is the switched-off build's, which is the whole
    grid's switched-off rule on those planes."""
    c, first = _case_series(abz, 3)
    on, off = _on_and_off(abz, monkeypatch, c, first, npt, kshard=kshard)
    assert 0 < on["eig"].shape[0] < npt**3 and on["eig"].shape[0] % (npt * npt) == 0
    _assert_same(on, off)


def test_update_real_complex_real(abz, monkeypatch):
    """update() re-detects the flag: real -> complex Hermitian -> real, every rebuild equals a fresh rule of those coefficients."""
    L = abz._lib
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ABZ_EVAL_MIRROR", "1")
    npt = 33
    rng = np.random.default_rng(4190)
    c_real, first = _real_hermitian(rng, DIMS, 3)
    a = rng.standard_normal(DIMS + (3, 3))
    c_cplx = c_real + 0.5j * (a - np.swapaxes(a[::-1, ::-1, ::-1], -1, -2))  # Hermitian, not real
    assert np.array_equal(c_cplx, np.conj(np.swapaxes(c_cplx[::-1, ::-1, ::-1], -1, -2))) and np.abs(c_cplx.imag).max() > 0
    c_real2, _ = _real_hermitian(rng, DIMS, 3)
    fresh = [_rule_data(abz, c, first, npt) for c in (c_real, c_cplx, c_real2)]
    dev = abz.FourierSeries(c_real, period=1.0, first=first, ndim=3).device()
    try:
        rule = dev.rule(npt, None, L.WANT_H | L.WANT_EIG)
        _assert_same(rule.export(x=False, w=False, H=True, eig=True), fresh[0])
        for c, want in ((c_cplx, fresh[1]), (c_real2, fresh[2])):
            dev.update(c)
            rule.rebuild()
            _assert_same(rule.export(x=False, w=False, H=True, eig=True), want)
        rule.close()
    finally:
        dev.drop_rules()
    # the complex rule is the one every plane of which is evaluated; the real ones are mirrored
    g = _grid(fresh[1]["H"], npt)
    assert not np.array_equal(g[npt // 2 + 1:], np.conj(_at_minus_k(g)[npt // 2 + 1:]))
    for f in (fresh[0], fresh[2]):
        g = _grid(f["H"], npt)
        assert np.array_equal(g[npt // 2 + 1:], np.conj(_at_minus_k(g)[npt // 2 + 1:]))

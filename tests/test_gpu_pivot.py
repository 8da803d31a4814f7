"""ABZ_PIVOT_PARTIAL on the device: the row-pivoted Gauss-Jordan of big_inverse_kernel against the long-double reference on
series whose resolvent cannot be eliminated without pivoting (tests/pivot_cases.py: the pivot of every node is exactly
omega at eta = 0, NaN at omega = 0 in the default mode), through every route that takes the mode.

Bound: every component finite and within K_BOUND eps A of the reference (A: resolvent_ref.amplification, over pi for a DOS) --
group (b) "A" of test_gpu_resolvent_edges.py; LAPACK's own route sits at <= 0.3 eps A on these cases.  `-s` prints the worst
err / (eps A) per band group at the end of the bound tests.
"""
import numpy as np
import pytest

import abz_oracle as orc
import pivot_cases as pc
import resolvent_ref as rr

pytestmark = pytest.mark.gpu

K = rr.K_BOUND
ORIGIN_TOL = 1e-11  # test_gpu_resolvent_edges.py, group (a)


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def _fids(L):
    return {"dos": L.F_DOS, "trgloc": L.F_TRGLOC, "gloc": L.F_GLOC}


def _group(n):
    return "1-4" if n <= 4 else ("5-8" if n <= 8 else ("9-16" if n <= 16 else ("17-32" if n <= 32 else "33-64")))


def _sel(case, ns):
    return slice(case.one, case.one + 1) if ns == 1 else slice(None)


def _series(abz, case, mode=None):
    s = abz.FourierSeries(case.c, period=1.0, first=case.first, ndim=case.d)
    return s, s.device(pivoting=mode)


def _routes(abz, case, dev, herm, want=None):
    """{(route, kind, n_sweep): complex [n_sweep, ncomp]}: a WANT_H rule (and eigenvalues for a Hermitian series) and the
    store-free sum where the library serves it, the three resolvent integrands, a sweep of one value and of all five."""
    L = abz._lib
    out = {}
    rule = abz.DeviceRule(dev, case.npt, None, want if want is not None else (L.WANT_H | (L.WANT_EIG if herm else 0)))
    for sweep in (case.sweep[_sel(case, 1)], case.sweep):
        for kind, fid in _fids(L).items():
            out[("reduce", kind, len(sweep))] = rule.reduce(fid, [case.eta], sweep)
            if dev.ptr_sum_supported(case.npt, fid):  # (the only skip: a route the library does not serve)
                out[("ptr_sum", kind, len(sweep))] = dev.ptr_sum(case.npt, fid, [case.eta], sweep)
    rule.close()
    return out


def _check(case, res):
    """[(route, kind, ns, err / (eps A))] of the results that are not finite or miss K eps A, and the worst ratio of all."""
    bad, worst = [], 0.0
    for (route, kind, ns), got in sorted(res.items()):
        unit = rr.EPS * case.amp[_sel(case, ns)] / (np.pi if kind == "dos" else 1.0)
        ref = np.asarray(case.ref(kind)[_sel(case, ns)])
        finite = bool(np.isfinite(got.view(np.float64)).all())
        err = np.abs(got.astype(np.clongdouble) - ref).max(axis=1).astype(np.float64) if finite else np.full(ns, np.nan)
        r = float((err / unit).max())
        print(f"{case.name} {route:7s} {kind:7s} sweep of {ns}: err / (eps A) {r:9.3g}")
        worst = max(worst, r) if finite else float("inf")
        if not (finite and (err <= K * unit).all()):
            bad.append((route, kind, ns, r))
    return bad, worst


_ALL = pc.all_cases()
_WORST = {}


@pytest.mark.parametrize("p", _ALL, ids=[pc.case_id(p) for p in _ALL])
def test_pivoted_routes_within_bound(abz, p):
    case = pc.get(p)
    herm = p[0] == "paired"
    s, dev = _series(abz, case, "partial")
    assert dev.hermitian() == herm and dev.pivoting() == "partial"
    res = _routes(abz, case, dev, herm)
    dev.close()
    # every route is served in this mode: 2 routes x 3 kinds x 2 sweeps
    assert len(res) == 12, sorted(res)
    bad, worst = _check(case, res)
    key = (p[0], _group(case.n))
    _WORST[key] = max(_WORST.get(key, 0.0), worst)
    assert not bad, bad


def test_zz_print_worst_per_band_group():
    """(runs after the cases above: their worst err / (eps A) per family and band group, for DESIGN section 9)"""
    for (fam, grp), w in sorted(_WORST.items()):
        print(f"worst err / (eps A), {fam:12s} {grp:6s} bands: {w:.3g}")
    assert all(w <= K for w in _WORST.values())


def test_default_mode_fails_where_pivoting_is_needed(abz):
    """What the mode is for: the same scan in mode "none" is not finite at omega = 0 (8-band shift family), and is with
    "partial" -- on one rule, built before the mode was set."""
    L = abz._lib
    case = pc.get(("shift", 8, None, None))
    s, dev = _series(abz, case)
    assert dev.pivoting() == "none"
    rule = abz.DeviceRule(dev, case.npt, None, L.WANT_H)
    zero = case.sweep[_sel(case, 1)]
    assert not np.isfinite(rule.reduce(L.F_TRGLOC, [0.0], zero).view(np.float64)).all()
    dev.set_pivoting("partial")
    got = rule.reduce(L.F_TRGLOC, [0.0], zero)  # (the rule was built before the call)
    assert np.abs(got.astype(np.clongdouble) - np.asarray(case.ref("trgloc")[_sel(case, 1)])).max() <= K * rr.EPS * case.amp[case.one]
    rule.close()
    dev.close()


# ------------------------------------------------------------------------------------------- dissipative: both modes valid
_DISS = (3, 8, 16, 32, 64)
_DISS_RES = {}


def _diss(abz, n):
    """Results of the dissipative case in the order none, partial, partial again, none again."""
    if n not in _DISS_RES:
        case = rr.origin_case(n, False)
        s, dev = _series(abz, case)
        runs = []
        for mode in (None, "partial", "partial", "none"):
            if mode is not None:
                dev.set_pivoting(mode)
            runs.append(_routes(abz, case, dev, False))
        dev.close()
        _DISS_RES[n] = (case, runs)
    return _DISS_RES[n]


@pytest.mark.parametrize("n", _DISS)
def test_pivoting_does_not_hurt(abz, n):
    case, runs = _diss(abz, n)
    bad = []
    for (route, kind, ns), got in sorted(runs[1].items()):
        ref = np.asarray(case.ref(kind)[_sel(case, ns)])
        scale = float(np.abs(ref).max())
        finite = bool(np.isfinite(got.view(np.float64)).all())
        err = float(np.abs(got.astype(np.clongdouble) - ref).max()) if finite else float("nan")
        print(f"{case.name} {route:7s} {kind:7s} sweep of {ns}: err / max|ref| {err / scale:.2e}")
        if not (finite and err <= ORIGIN_TOL * scale):
            bad.append((route, kind, ns, err / scale))
    assert not bad, bad


@pytest.mark.parametrize("n", _DISS)
def test_default_untouched_and_repeats_bit_identical(abz, n):
    case, (none0, part0, part1, none1) = _diss(abz, n)
    assert sorted(part0) == sorted(part1) and set(none0) <= set(part0) and sorted(none0) == sorted(none1)
    for key in none0:
        assert np.array_equal(none0[key].view(np.float64), none1[key].view(np.float64)), key  # none, then partial -> none
    for key in part0:
        assert np.array_equal(part0[key].view(np.float64), part1[key].view(np.float64)), key  # the same call twice


# ----------------------------------------------------------------------------------------------------------- mode plumbing
def test_mode_round_trip_update_and_bad_mode(abz):
    case = pc.get(("shift", 5, None, None))
    s, dev = _series(abz, case)
    assert dev.pivoting() == "none"
    dev.set_pivoting("partial")
    assert dev.pivoting() == "partial"
    dev.update(case.c)
    assert dev.pivoting() == "partial"  # update() keeps the mode
    assert s.device() is dev and s.device().pivoting() == "partial"  # None leaves it alone
    assert s.device(pivoting="none").pivoting() == "none"
    with pytest.raises(ValueError):
        dev.set_pivoting("complete")
    with pytest.raises(ValueError):
        s.device(pivoting="rows")
    L = abz._lib
    assert L.lib().abz_series_set_pivoting(dev.h, 2) == L.ERR_ARG
    assert dev.pivoting() == "none"
    dev.close()


def test_rule_without_h_is_refused(abz):
    L = abz._lib
    case = pc.get(("paired", 8, None, None))
    s, dev = _series(abz, case, "partial")
    rule = abz.DeviceRule(dev, case.npt, None, L.WANT_EIG)
    with pytest.raises(abz.AbzError, match="ABZ_WANT_H"):
        rule.reduce(L.F_DOS, [0.0], case.sweep)
    got = rule.reduce(L.F_DOS_EIG, [0.05], case.sweep)  # other integrands are untouched
    assert np.isfinite(got.view(np.float64)).all()
    rule.close()
    dev.close()


def test_autoptr_through_the_integrand_keyword(abz):
    """One AutoPTR solve of tr G at omega = 0 on the 5-band shift family, d = 1: the integrand's keyword sets the mode of the
    device copy, and the solve returns the rule value of the grid it stopped on."""
    L = abz._lib
    case = pc.shift_case(5, 1, 7)
    s = abz.FourierSeries(case.c, period=1.0, first=case.first, ndim=1)
    bz = abz.load_bz(abz.FBZ(), np.eye(1))
    sol = abz.do_solve(abz.FourierIntegrand(abz.TrGlocIntegrand(pivoting="partial"), s, 0.0), bz, abz.MixedParameters(0.0),
                       abz.AutoPTR(), abstol=1e-10)
    dev = s.device()
    assert dev.pivoting() == "partial"
    u = sol.u / abs(np.linalg.det(bz.B))  # (the solve applies |det B|; the rule value is per unit cell)
    npt = sol.extra["npt"]
    rule = abz.DeviceRule(dev, npt, None, L.WANT_H)
    val = rule.reduce(L.F_TRGLOC, [0.0], [0.0])[0, 0]
    rule.close()
    dev.close()
    Hk = rr.fourier_nodes(case.c, case.first, npt, 1)
    A = rr.amplification(Hk, np.ones(len(Hk)), 0.0)
    ref = complex(rr.rule_sum(Hk, np.ones(len(Hk)), 0.0, "trgloc"))
    print(f"AutoPTR stopped at npt = {npt}: |solve - reduce| / (eps A) {abs(u - val) / (rr.EPS * A):.3g}")
    assert np.isfinite(u) and abs(u - val) <= 2 * K * rr.EPS * A  # (each is within K eps A of the exact rule value)
    assert abs(u - ref) <= K * rr.EPS * A


def test_iai_solves_through_the_pivoted_node_values(abz):
    """IAI above 4 bands in this mode keeps its innermost loops on the host and takes the node values from the pivoted
    inverse (node mode of big_inverse_kernel): the 5-band shift family in 2-D against the oracle, whose `inv` pivots."""
    case = pc.get(("shift", 5, None, None))
    s = abz.FourierSeries(case.c, period=1.0, first=case.first, ndim=2)
    so = orc.FourierSeries(case.c, period=1.0, first=case.first, ndim=2)
    bz = abz.load_bz(abz.FBZ(), np.eye(2))
    sol = abz.do_solve(abz.FourierIntegrand(abz.TrGlocIntegrand(pivoting="partial"), s, 0.0), bz, abz.MixedParameters(0.0),
                       abz.EvalCounter(abz.IAI()), abstol=1e-3)
    f_tr = lambda x, h: np.trace(orc.f_gloc(0.0, 0.0)(x, h), axis1=-2, axis2=-1)
    ref = orc.solve_iai(so, orc.load_bz("FBZ", np.eye(2)), f_tr, abstol=1e-3)
    s.device().close()
    assert np.isfinite(sol.u)
    assert sol.numevals == ref.numevals and abs(sol.u - ref.u) <= 1e-9 * abs(ref.u)


def test_gloc_node_values_are_pivoted(abz):
    """abz_eval_line_nodes, F_GLOC: the matrix-valued node mode stores to permuted addresses (17 bands: two nodes per wave)."""
    L = abz._lib
    case = pc.get(("derangement", 17, None, None))
    s, dev = _series(abz, case, "partial")
    x = np.arange(case.npt) / case.npt
    got = dev.eval_line_nodes(np.zeros(len(x), dtype=np.int64), x, L.F_GLOC, [0.0], 0.0).reshape(len(x), case.n, case.n)
    dev.close()
    G, _ = rr.refined_inverse(-case.Hk)  # z = 0
    amp = np.array([rr.amplification(case.Hk[k:k + 1], np.ones(1), 0.0) for k in range(len(x))])
    err = np.abs(np.swapaxes(got, -1, -2).astype(np.clongdouble) - G).max(axis=(-2, -1)).astype(np.float64)
    print(f"{case.name} node values of G: err / (eps A) {(err / (rr.EPS * amp)).max():.3g}")
    assert np.isfinite(got.view(np.float64)).all() and (err <= K * rr.EPS * amp).all()


# ----------------------------------------------------------------------------------------------------------- compact rules
@pytest.mark.parametrize("n", (4, 16))
def test_compact_rule_is_expanded_on_load(abz, n):
    """A rule that keeps the upper triangle of a Hermitian H(k) only: the pivoted scan expands it as it loads -- the same
    matrices as the full layout bit for bit, so the same sums."""
    L = abz._lib
    case = pc.get(("paired", n, None, None))
    s, dev = _series(abz, case, "partial")
    rule = abz.DeviceRule(dev, case.npt, None, L.WANT_H | L.WANT_H_COMPACT)
    assert rule.want & L.WANT_H_COMPACT
    full = abz.DeviceRule(dev, case.npt, None, L.WANT_H)
    assert not full.want & L.WANT_H_COMPACT
    res = {}
    for kind, fid in _fids(L).items():
        res[("reduce", kind, 5)] = rule.reduce(fid, [0.0], case.sweep)
        assert np.array_equal(res[("reduce", kind, 5)].view(np.float64), full.reduce(fid, [0.0], case.sweep).view(np.float64))
    rule.close()
    full.close()
    dev.close()
    bad, _ = _check(case, res)
    assert not bad, bad

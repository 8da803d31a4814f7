"""The resolvent kernels where they can lose digits: eta = 0 at the origin of a gapped or dissipative spectrum, a pole at
1e-2 ... 1e-6 of the spectral radius, and the agreement of the routes with each other there.  Default dispatch only (no
switch is set): what a user gets.  The reference is tests/resolvent_ref.py (inverses refined in long double); the bounds
are multiples of eps * A, A the case's own amplification of an input perturbation (resolvent_ref.amplification).

Band counts, one or two per kernel family (Hermitian series / series that are not):
    1, 2, 3, 4    closed forms / big_inverse_kernel<1, 8> (store-free sums of a grid line of <= 128 points, and every
                  store-free sum of a series that is not Hermitian)
    5, 8          one node per lane / big_inverse_kernel<2, 8>
    12, 16        16-lane row kernels / big_inverse_kernel<3, 4>, <4, 4>
    17, 24, 32    32-lane row kernels / big_inverse_kernel<5...8, 2>
    33, 48, 64    tridiagonal chunk sums / big_inverse_kernel<10...16, 1>
Routes: DeviceRule.reduce on a cached rule (H, and eigenvalues for a Hermitian series) and DeviceSeries.ptr_sum, for
F_DOS, F_TRGLOC, F_GLOC (F_DOS_EIG where the rule holds eigenvalues); a sweep of one value and a sweep of five (five
values select the tridiagonal routes up to 16 bands, and 5 is no multiple of a lane count).

Which route is held to which bound in group (b), with the measured err / (eps A), is the table HELD below.
"""
import numpy as np
import pytest

import resolvent_ref as rr

pytestmark = pytest.mark.gpu

K = rr.K_BOUND
ORIGIN_TOL = 1e-11  # the suite's parity tolerance: the cases of group (a) are well conditioned (cond <= 1e3, asserted)


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def _group(n):
    return "1-4" if n <= 4 else ("5-8" if n <= 8 else ("9-16" if n <= 16 else ("17-32" if n <= 32 else "33-64")))


# Group (b): the bound a route is held to.  "A": K eps A.  "doc": K eps A max_k ||z - H_k||_2 / eta, what the header of
# kernels_generic.hip documents for the routes that eliminate without pivoting (Gauss-Jordan row kernels,
# big_inverse_kernel, the p'/p recurrence); a route is listed here only because it misses "A", and none may need "doc" at
# eta / rho = 1e-2.  Key: (band group, "herm" | "diss", route, kind, eta / rho); everything not listed is held to "A".
# No route is listed and no figure stands here: the worst err / (eps A) per route, which `-s` prints, has not been recorded.
HELD = {
}


def _held(n, herm, route, kind, ratio):
    return HELD.get((_group(n), "herm" if herm else "diss", route, kind, ratio), "A")


_CASES = {}


def _case(fn, *args):
    key = (fn.__name__,) + args
    if key not in _CASES:
        _CASES[key] = fn(*args)
    return _CASES[key]


_RESULTS = {}


def _served(dev, n, npt, fid, L):
    """The store-free sums abz_ptr_sum serves: what ptr_sum_supported reports, and up to 4 bands the inverse of every node
    wherever the closed-form kernel does not apply (a short grid line, a series that is not Hermitian).
    DeviceSeries.ptr_sum_supported understates the library there: it answers for the closed-form kernel only."""
    return dev.ptr_sum_supported(npt, fid) or (n <= 4 and fid in (L.F_DOS, L.F_TRGLOC, L.F_GLOC))


def _sel(case, ns):
    """The part of the case's five swept values that a sweep of `ns` values holds (one value: case.one, else all)."""
    return slice(case.one, case.one + 1) if ns == 1 else slice(None)


def _run(abz, key, case, herm):
    """{(route, kind, n_sweep): complex [n_sweep, ncomp]} of one case, both routes, a sweep of one value and of all five."""
    if key in _RESULTS:
        return _RESULTS[key]
    L = abz._lib
    fids = {"dos": L.F_DOS, "trgloc": L.F_TRGLOC, "gloc": L.F_GLOC}
    s = abz.FourierSeries(case.c, period=1.0, first=case.first, ndim=case.d)
    dev = s.device()
    assert dev.hermitian() == herm
    out = {}
    rule = abz.DeviceRule(dev, case.npt, None, L.WANT_H | (L.WANT_EIG if herm else 0))
    for sweep in (case.sweep[_sel(case, 1)], case.sweep):
        for kind, fid in fids.items():
            out[("reduce", kind, len(sweep))] = rule.reduce(fid, [case.eta], sweep)
        if herm:
            out[("reduce", "dos_eig", len(sweep))] = rule.reduce(L.F_DOS_EIG, [case.eta], sweep)
    rule.close()
    for sweep in (case.sweep[_sel(case, 1)], case.sweep):
        for kind, fid in fids.items():
            if _served(dev, case.n, case.npt, fid, L):
                out[("ptr_sum", kind, len(sweep))] = dev.ptr_sum(case.npt, fid, [case.eta], sweep)
    dev.drop_rules()
    _RESULTS[key] = out
    return out


def _ref(case, kind, ns):
    return np.asarray(case.ref("dos" if kind == "dos_eig" else kind)[_sel(case, ns)])


def _err(got, case, kind, ns):
    """[ns] largest |got - ref| over the components, in float64 (the difference taken in long double)."""
    return np.abs(got.astype(np.clongdouble) - _ref(case, kind, ns)).max(axis=1).astype(np.float64)


_ORIGIN = ([(n, h, None, None) for h in (True, False) for n in rr.BANDS] +
           [(n, h, d, npt) for h in (True, False) for n, d, npt in rr.RAGGED] +
           [(n, True, d, npt) for n, d, npt in rr.LONG_LINE])


def _oid(p):
    n, h, d, npt = p
    return f"{n}-{'herm' if h else 'diss'}" + (f"-{d}d{npt}" if d else "")


@pytest.mark.parametrize("p", _ORIGIN, ids=[_oid(p) for p in _ORIGIN])
def test_origin(abz, p):
    """(a) eta = 0, swept values [0] and [-0.25, 0, 0.1, 0.25, 0.4] gap: a gapped Hermitian series, or a dissipative one
    (Gamma >= 0.1).  Every number finite and within 1e-11 max|ref|; the Hermitian DOS inside the gap, whose reference is 0
    itself, is 0 to 1e-11 max|tr G|.  The store-free sums and the scans that go through
    big_inverse_kernel returned NaN here before its empty sub-slots were given the identity."""
    n, herm, d, npt = p
    case = _case(rr.origin_case, n, herm) if d is None else _case(rr.origin_case, n, herm, d, npt)
    assert case.cond <= 1e3, case.cond
    assert case.residual <= 1e-15
    assert case.sweep[case.one] == 0.0  # the sweep of one value is the origin itself
    res = _run(abz, p, case, herm)
    bad = []
    for (route, kind, ns), got in sorted(res.items()):
        ref = _ref(case, kind, ns)
        finite = bool(np.isfinite(got.view(np.float64)).all())
        if herm and kind in ("dos", "dos_eig"):
            # inside the gap the DOS is 0 and so is max|ref|: it is 0 to 1e-11 of tr G, whose imaginary part it is
            scale, what = float(np.abs(_ref(case, "trgloc", ns)).max()), "|DOS| / max|tr G|"
            err = float(np.abs(got).max()) if finite else float("nan")
        else:
            scale, what = float(np.abs(ref).max()), "err / max|ref|"
            err = float(np.abs(got.astype(np.clongdouble) - ref).max()) if finite else float("nan")
        print(f"{case.name} {route:7s} {kind:7s} sweep of {ns}: {what} {err / scale:.2e}")
        if not (finite and err <= ORIGIN_TOL * scale):
            bad.append((route, kind, ns, err / scale))
    assert not bad, bad


_SMALL = ([(n, h, r, None, None) for h in (True, False) for n in rr.BANDS for r in rr.RATIOS] +
          [(n, True, r, d, npt) for n, d, npt in rr.LONG_LINE for r in rr.RATIOS] +
          [(n, h, rr.RAGGED_RATIO, d, npt) for h in (True, False) for n, d, npt in rr.RAGGED])


def _sid(p):
    n, h, r, d, npt = p
    return f"{n}-{'herm' if h else 'diss'}-{r:g}" + (f"-{d}d{npt}" if d else "")


def _small_case(p):
    n, herm, ratio, d, npt = p
    return _case(rr.small_eta_case, n, herm, ratio) if d is None else _case(rr.small_eta_case, n, herm, ratio, d, npt)


def _bounds(case, n, herm, route, kind, ratio, ns):
    """[ns] the bound the route is held to, and eps A (over pi for a DOS, which is -Im tr G / pi)."""
    unit = rr.EPS * case.amp[_sel(case, ns)] / (np.pi if kind in ("dos", "dos_eig") else 1.0)
    if _held(n, herm, route, kind, ratio) == "A":
        return K * unit, unit
    # the documented bound of the unpivoted routes: the growth factor ||z - H_k|| / eta
    dist = ratio * rr.spectral_radius(case.Hk) if not herm else case.eta
    growth = np.array([np.linalg.norm(complex(om, case.eta) * np.eye(n) - case.Hk, 2, axis=(-2, -1)).max() / dist
                       for om in case.sweep[_sel(case, ns)]])
    return K * unit * growth, unit


@pytest.mark.parametrize("p", _SMALL, ids=[_sid(p) for p in _SMALL])
def test_small_eta(abz, p):
    """(b) a pole at eta / rho = 1e-2, 1e-4, 1e-6 of one node (pole_sweep): |got - ref| <= K eps A, K = max(64,
    8 r_lapack); the routes listed in HELD: K eps A ||z - H_k|| / eta."""
    n, herm, ratio, d, npt = p
    case = _small_case(p)
    res = _run(abz, p, case, herm)
    bad = []
    for (route, kind, ns), got in sorted(res.items()):
        bound, unit = _bounds(case, n, herm, route, kind, ratio, ns)
        assert (case.ref_err[_sel(case, ns)] <= bound / 64).all()  # the reference's own error is far below what it judges
        finite = bool(np.isfinite(got.view(np.float64)).all())
        err = _err(got, case, kind, ns) if finite else np.full(ns, np.nan)
        r = float((err / unit).max())
        print(f"{case.name} {route:7s} {kind:7s} sweep of {ns}: err / (eps A) {r:9.3g}  held to {_held(n, herm, route, kind, ratio)}")
        if not (finite and (err <= bound).all()):
            bad.append((route, kind, ns, r))
    assert not bad, bad


_CONS = [p for p in _SMALL if p[2] == 1e-4]


@pytest.mark.parametrize("p", _CONS, ids=[_sid(p) for p in _CONS])
def test_consistency(abz, p):
    """(c) at eta / rho = 1e-4: reduce and ptr_sum agree within twice the bound, and a sweep of five values returns at its
    first value what the sweep of that one value returns (other kernels serve the two sweeps up to 16 bands)."""
    n, herm, ratio, d, npt = p
    case = _small_case(p)
    res = _run(abz, p, case, herm)
    bad = []
    for (route, kind, ns), got in sorted(res.items()):
        if ns != 5:
            continue
        b5 = _bounds(case, n, herm, route, kind, ratio, 5)[0]
        one = res[(route, kind, 1)]
        dif = float(np.abs(got[case.one] - one[0]).max())
        print(f"{case.name} {route:7s} {kind:7s} five vs one: {dif / b5[case.one]:.3g} of the bound")
        if not dif <= 2.0 * b5[case.one]:
            bad.append((route, kind, "five vs one", dif / b5[case.one]))
        if route == "reduce" and ("ptr_sum", kind, 5) in res:
            bo = np.maximum(b5, _bounds(case, n, herm, "ptr_sum", kind, ratio, 5)[0])
            for m in (1, 5):
                dif = np.abs(res[("reduce", kind, m)] - res[("ptr_sum", kind, m)]).max(axis=1)
                rel = float((dif / bo[_sel(case, m)]).max())
                print(f"{case.name} {kind:7s} reduce vs ptr_sum, sweep of {m}: {rel:.3g} of the bound")
                if not rel <= 2.0:
                    bad.append((kind, "reduce vs ptr_sum", m, rel))
    assert not bad, bad

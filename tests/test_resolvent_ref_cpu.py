"""The high-precision resolvent reference (tests/resolvent_ref.py) checked by itself: its inverse against mpmath at 50
digits, its case builders against their promises, and the error of the plain complex128 route over every case of the GPU
test (the r_lapack that enters the GPU bound)."""
import numpy as np
import pytest

import resolvent_ref as rr


def _mp_inverse(A):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    n = A.shape[0]
    M = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            M[i, j] = mp.mpc(float(A[i, j].real), float(A[i, j].imag))
    X = M ** -1
    return X


def _against_mpmath(A, tol):
    X, res = rr.refined_inverse(A, tol)
    Xm = _mp_inverse(A)
    mp = pytest.importorskip("mpmath")
    n = A.shape[0]
    scale = max(abs(Xm[i, j]) for i in range(n) for j in range(n))
    err = 0.0
    for i in range(n):
        for j in range(n):
            # the long double entry enters mpmath exactly as the sum of its float64 head and tail
            re, im = X[i, j].real, X[i, j].imag
            hr, hi = np.float64(re), np.float64(im)
            got = mp.mpc(mp.mpf(float(hr)) + mp.mpf(float(re - hr)), mp.mpf(float(hi)) + mp.mpf(float(im - hi)))
            err = max(err, float(abs(got - Xm[i, j]) / scale))
    return err, res


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("ratio", [1e-2, 1e-6])
def test_refined_inverse_against_mpmath(n, ratio):
    rng = np.random.default_rng([7, n])
    H = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    H = 0.5 * (H + H.conj().T)
    e = np.linalg.eigvalsh(H)
    rho = np.abs(e).max()
    A = complex(e[n // 2], ratio * rho) * np.eye(n) - H  # the pole at distance ratio * rho
    cond = np.linalg.cond(A)
    # the residual's floor is 2^-64 n cond (refined_inverse); the relative error of X is the residual
    floor = 2.0 ** -64 * 4 * n * cond
    err, res = _against_mpmath(A, tol=max(1e-15, floor))
    print(f"n={n} eta/|H|={ratio:g} cond {cond:.2e} residual {res:.1e} err vs mpmath {err:.1e}")
    assert res <= max(1e-15, floor)
    assert err <= max(4 * 2.0 ** -64 * n, 2.0 * res)


def test_refined_inverse_at_the_origin_of_a_gapped_matrix():
    c, first = rr.gapped_hermitian(np.random.default_rng(11), (3, 3), 8, rr.GAP)
    Hk = rr.fourier_nodes(c, first, 5, 2)
    err, res = _against_mpmath(-Hk[7], 1e-15)  # z = 0
    assert res <= 1e-15 and err <= 64 * 2.0 ** -64


def test_refined_inverse_refuses_what_it_cannot_refine():
    rng = np.random.default_rng(9)
    U, _ = np.linalg.qr(rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8)))
    V, _ = np.linalg.qr(rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8)))
    A = (U * np.array([1.0] * 7 + [1e-10])) @ V  # cond 1e10: the residual cannot fall below about 1e-9 in long double
    with pytest.raises(ArithmeticError):
        rr.refined_inverse(A)


@pytest.mark.parametrize("n", [1, 2, 5, 12, 33])
def test_gapped_hermitian_keeps_its_gap(n):
    d, npt = 2, 5
    c, first = rr.gapped_hermitian(np.random.default_rng([3, n]), (3, 3), n, rr.GAP)
    Hk = rr.fourier_nodes(c, first, npt, d)
    assert np.abs(Hk - np.conj(np.swapaxes(Hk, -1, -2))).max() <= 1e-15
    e = np.linalg.eigvalsh(Hk)
    assert np.abs(e).min() >= 0.5 * rr.GAP, np.abs(e).min()
    if n >= 2:  # states on both sides of the gap, so that 0 lies inside the spectrum
        assert e.min() < 0.0 < e.max()
    flip = c[::-1, ::-1]
    assert np.array_equal(c, np.conj(np.swapaxes(flip, -1, -2)))  # exactly: the library's own test for a Hermitian series


@pytest.mark.parametrize("n", [1, 2, 5, 12, 33])
@pytest.mark.parametrize("gamma", [0.1, 1e-6])
def test_dissipative_keeps_its_lower_bound(n, gamma):
    d, npt = 2, 5
    c, first = rr.dissipative(np.random.default_rng([4, n]), (3, 3), n, gamma)
    Hk = rr.fourier_nodes(c, first, npt, d)
    Gam = (Hk - np.conj(np.swapaxes(Hk, -1, -2))) / (-2j)  # H = H_h - i Gamma
    # (the Fourier sum leaves Gamma with an error of eps |H| per node)
    assert np.linalg.eigvalsh(Gam).min() >= gamma - 8 * rr.EPS * np.abs(Hk).max()
    c0, _ = rr.dissipative(np.random.default_rng([4, n]), (3, 3), n, 2.0 * gamma)
    Hk0 = rr.fourier_nodes(c0, first, npt, d)
    Hh = 0.5 * (Hk + np.conj(np.swapaxes(Hk, -1, -2)))
    Hh0 = 0.5 * (Hk0 + np.conj(np.swapaxes(Hk0, -1, -2)))
    assert np.abs(Hh - Hh0).max() <= 8 * rr.EPS * np.abs(Hk).max()  # the Hermitian part does not depend on gamma


def test_pole_sweep_places_its_values():
    c, first = rr.gapped_hermitian(np.random.default_rng(5), (3, 3), 6, rr.GAP)
    Hk = rr.fourier_nodes(c, first, 5, 2)
    sw = rr.pole_sweep(Hk, 12, 1e-4)
    e = np.linalg.eigvalsh(Hk[12])
    assert sw[0] in e and sw[3] in e and sw[0] != sw[3]
    assert np.abs(sw[1] - e).min() >= 0.25 * np.diff(e).max()
    assert sw[2] > np.linalg.eigvalsh(Hk).max()
    assert len(sw) == 5


def test_amplification_of_a_normal_matrix():
    rng = np.random.default_rng(6)
    n = 5
    H = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    H = 0.5 * (H + H.conj().T)
    z = 0.3 + 0.01j
    lam = np.linalg.eigvalsh(H)
    want = (np.linalg.norm(H) + abs(z)) * (1.0 / np.abs(z - lam) ** 2).sum()
    assert abs(rr.amplification(H[None], [1.0], z) - want) <= 1e-10 * want


def test_rule_sum_kinds_agree():
    c, first = rr.gapped_hermitian(np.random.default_rng(8), (3,), 4, rr.GAP)
    Hk = rr.fourier_nodes(c, first, 7, 1)
    w = np.ones(7)
    z = 0.05 + 0.02j
    G = rr.rule_sum(Hk, w, z, "gloc")
    lam = np.linalg.eigvalsh(Hk)
    tr = (1.0 / (z - lam)).sum(axis=1).mean()
    assert abs(complex(rr.rule_sum(Hk, w, z, "trgloc")) - tr) <= 1e-13 * abs(tr)
    assert abs(complex(np.trace(G)) - tr) <= 1e-13 * abs(tr)
    assert abs(float(rr.rule_sum(Hk, w, z, "dos")) + tr.imag / np.pi) <= 1e-13 * abs(tr)


_CASES = rr.edge_cases()


@pytest.mark.parametrize("fn,args", _CASES, ids=[f"{f.__name__}-{'-'.join(str(a) for a in args)}" for f, args in _CASES])
def test_r_lapack(fn, args):
    """err(numpy complex128 route) / (eps A) against the refined value, over every case of the GPU test: at most the
    committed R_LAPACK.  Also what the GPU test takes for granted about its reference: the refined value's own error
    bound is below 1/64 of the smallest bound a device route is held to."""
    case = fn(*args)
    r = 0.0
    for kind in rr.KINDS:
        err = np.abs(case.lapack(kind) - case.ref(kind)).max(axis=1).astype(np.float64)
        if kind == "dos":
            err = err * np.pi
        r = max(r, float((err / (rr.EPS * case.amp)).max()))
    print(f"{case.name}: cond {case.cond:.2e} residual {case.residual:.1e} r_lapack {r:.4f}")
    assert r <= rr.R_LAPACK
    assert (case.ref_err <= rr.K_BOUND * rr.EPS * case.amp / np.pi / 64).all()

"""Band expectation values as matrix elements of the tetrahedron method, CPU side: the bindings of abz_rule_ltm_expectation,
what LTM and BandExpectation accept, FourierSeries.derivative and velocity_operators against the oracle and a finite
difference, and the numpy restatement of the device tests (tests/expect_numpy.py) against a closed form.  The kernels are
checked in test_gpu_ltm_expectation.py."""
import inspect
import os
import re

import numpy as np
import pytest

import abz_oracle as orc
import expect_numpy as xn
import wltm_numpy as wn
from test_gpu_parity import rand_series

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0**-52


# ---------------------------------------------------------------- 1. bindings
def test_ltm_expectation_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert re.search(r"^int abz_rule_ltm_expectation\(abz_rule\* r, abz_rule\* const\* ops, int nops,\s*const int32_t\* comps(?: /\*.*?\*/)?, "
                     r"int ncomp\);", hdr, flags=re.M)
    assert "abz_rule_ltm_expectation" in L.PROTOTYPES
    assert hasattr(L.lib(), "abz_rule_ltm_expectation")
    assert ":abz_rule_ltm_expectation" in jl and "function ltm_expectation!" in jl
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_K_COUNT"] == 8 and defs["ABZ_VERSION"] == 502
    assert defs["ABZ_LTM_EXPECT_MAX_OPS"] == 8 == L.LTM_EXPECT_MAX_OPS and defs["ABZ_LTM_MAX_COMP"] == 16 == L.LTM_MAX_COMP
    for cls in (abz.DeviceRule, abz.UnfoldedRule):
        assert hasattr(cls, "ltm_expectation")
    assert list(inspect.signature(abz.DeviceRule.ltm_expectation).parameters) == ["self", "operators", "components"]
    assert list(inspect.signature(abz.velocity_operators).parameters) == ["h", "basis"]
    assert abz.BandExpectation is abz.dos.BandExpectation and abz.velocity_operators is abz.dos.velocity_operators
    assert "degenerate" in hdr[hdr.index("Band expectation values of operator series"):hdr.index("int abz_rule_ltm_expectation(")]


# ---------------------------------------------------------------- 2. what the algorithm accepts
def small_series(abz, d=1, n=2, seed=3):
    c, first = rand_series(np.random.default_rng(seed), (3,) * d, n, hermitian=True)
    return abz.FourierSeries(c, period=1.0, first=first, ndim=d)


def test_ltm_accepts_velocities_and_band_expectations():
    import autobzcore.jl_amd as abz
    s = small_series(abz)
    assert abz.LTM(elements="velocities").elements == "velocities"
    assert abz.LTM(elements="velocities", cumulative=True).cumulative
    assert abz.LTM(elements="velocities", eta=0.1).eta == 0.1
    be = abz.BandExpectation([s, s], [0, (0, 1), (1, 1), (1, -1)])
    assert be.components == ((0, -1), (0, 1), (1, 1), (1, -1)) and be.operators == (s, s)
    assert abz.BandExpectation(s).components is None and abz.BandExpectation(s).operators == (s,)
    assert abz.LTM(elements=be).elements is be
    for bad in ("bands", "velocity", 3):
        with pytest.raises(ValueError):
            abz.LTM(elements=bad)
    with pytest.raises(ValueError):
        abz.LTM(elements="velocities", eigenvectors="device")  # (that switch belongs to "orbitals")


def test_band_expectation_validates():
    import autobzcore.jl_amd as abz
    s = small_series(abz)
    with pytest.raises(ValueError, match="operators"):
        abz.BandExpectation([])
    with pytest.raises(ValueError, match="operators"):
        abz.BandExpectation([s] * 9)
    abz.BandExpectation([s] * 8, [(i % 8, 7 - i % 8) for i in range(16)])
    with pytest.raises(ValueError, match="components"):
        abz.BandExpectation([s] * 8, [0] * 17)
    with pytest.raises(ValueError, match="components"):
        abz.BandExpectation([s], [])
    for bad in ([1], [(0, 1)], [-1], [(0, -2)], [(2, 0)], [(0, 0, 0)], [0.5], [(0, 0.5)]):
        with pytest.raises(ValueError):
            abz.BandExpectation([s], bad)
    with pytest.raises(ValueError):
        abz.BandExpectation([s, s], [(0, 2)])


def test_expectations_need_the_unsymmetrised_grid():
    """symmetric=True on a symmetric zone is refused where the cache is made, before anything touches a device."""
    import autobzcore.jl_amd as abz
    s = small_series(abz, d=3)
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    for el in ("velocities", abz.BandExpectation([s])):
        with pytest.raises(ValueError, match="symmetric=False"):
            abz.dos.init(abz.DOSProblem(s, [0.0], cub), abz.LTM(npt=4, elements=el, symmetric=True))


# ---------------------------------------------------------------- 3. derivative series
@pytest.mark.parametrize("d", [1, 2, 3])
def test_derivative_series_matches_the_oracle(d):
    """FourierSeries.derivative(j) = the oracle's d/dx_j series times t_j, offsets != 0 and periods != 1.  The coefficients
    are one product each on both sides, in another order of the three factors: 4 eps of the largest coefficient."""
    import autobzcore.jl_amd as abz
    rng = np.random.default_rng(40 + d)
    dims, first, period = (3, 4, 5)[:d], (-1, 2, -4)[:d], (2.0, 0.5, 3.0)[:d]
    for n in (1, 3):
        c, _ = rand_series(rng, dims, n, first=first)
        s = abz.FourierSeries(c, period=period, first=first, ndim=d)
        so = orc.FourierSeries(c, period=period, first=first, ndim=d)
        for j in range(d):
            ds = s.derivative(j)
            ref = orc.derivative_series(so, j).c * so.t[j]
            assert ds.c.shape == s.c.shape and ds.first == s.first and ds.t == s.t and ds.d == d and ds.n == n
            assert np.abs(ds.c - ref).max() <= 4 * EPS * np.abs(ref).max()
    sc = abz.FourierSeries(rng.standard_normal(dims), period=period, first=first)
    assert sc.scalar and sc.derivative(0).scalar and sc.derivative(0).c.shape == sc.c.shape
    with pytest.raises(ValueError):
        s.derivative(d)
    # a Hermitian series keeps c(-R) = c(R)^dagger
    ch, fh = rand_series(rng, (3,) * d, 2, hermitian=True)
    dh = abz.FourierSeries(ch, period=1.0, first=fh, ndim=d).derivative(d - 1)
    flip = dh.c[tuple(slice(None, None, -1) for _ in range(d))]
    assert np.array_equal(dh.c, np.conj(np.swapaxes(flip, -1, -2)))


# ---------------------------------------------------------------- 4. Cartesian velocities
def test_velocity_operators_give_cartesian_band_velocities():
    """2-D oblique lattice A, B = 2 pi inv(A)^T, k = B kappa: with basis M = inv(B)^T = A / 2 pi the expectation <u_b|O_a|u_b> (numpy eigh on
    the oracle's host evaluation) is d e_b / d k_a, compared with the central difference (e_b(k + h e_a) - e_b(k - h e_a)) / 2h,
    h = 1e-4.  Two bands held apart by an on-site splitting of 6, so the eigenvalues are smooth.  Bound: the formula's own
    error term h^2 / 6 max|e'''| plus its rounding 16 eps max|e| / h; a non-degenerate eigenvalue has
    |e'''| <= ||H'''|| + 6 ||H'|| ||H''|| / gap + 12 ||H'||^3 / gap^2 (third-order perturbation theory, two bands), with
    ||d^m H / dk_a^m|| <= sum_R |2 pi R.M_a|^m ||c_R|| and the gap bounded below by the splitting minus twice the hopping
    norm."""
    import autobzcore.jl_amd as abz
    rng = np.random.default_rng(77)
    c, first = rand_series(rng, (3, 3), 2, hermitian=True)
    c *= 0.03
    c[1, 1] += np.diag([0.0, 6.0])
    A = np.array([[1.0, 0.4], [0.0, 0.9]])
    bz = abz.load_bz(abz.FBZ(), A)
    M = np.linalg.inv(bz.B).T  # M[a, j] = d kappa_j / d k_a
    assert np.allclose(M, A / (2 * np.pi)) and max(abs(M[0, 1]), abs(M[1, 0])) > 1e-2  # not diagonal
    h = abz.FourierSeries(c, period=1.0, first=first)
    ops = abz.velocity_operators(h, M)
    assert len(ops) == 2 and all(o.c.shape == h.c.shape and o.first == h.first and o.t == h.t for o in ops)
    ident = abz.velocity_operators(h)
    assert all(np.array_equal(ident[j].c, h.derivative(j).c) for j in range(2))
    with pytest.raises(ValueError):
        abz.velocity_operators(h, np.eye(3))
    so = orc.FourierSeries(c, period=1.0, first=first, ndim=2)
    oso = [orc.FourierSeries(o.c, period=1.0, first=first, ndim=2) for o in ops]
    kappa = rng.random((12, 2))
    q = xn.expectations(orc.evaluate_many(so, kappa), [orc.evaluate_many(o, kappa) for o in oso])  # [2, 12, 2]
    step = 1e-4
    R = np.stack(np.meshgrid(np.arange(-1, 2), np.arange(-1, 2), indexing="ij"), axis=-1).reshape(-1, 2)
    cn = np.linalg.norm(c.reshape(-1, 2, 2), 2, axis=(1, 2))
    hop = cn.sum() - cn[4]  # everything but R = 0
    gap = 6.0 - 2.0 * (hop + np.linalg.norm(c[1, 1] - np.diag([0.0, 6.0]), 2))
    assert gap > 4.0
    emax = 6.0 + cn.sum()
    for a in range(2):
        dk = np.zeros(2)
        dk[a] = step
        dkap = np.linalg.solve(bz.B, dk)  # kappa = inv(B) k
        ep = np.linalg.eigvalsh(orc.evaluate_many(so, kappa + dkap), UPLO="U")
        em = np.linalg.eigvalsh(orc.evaluate_many(so, kappa - dkap), UPLO="U")
        fd = (ep - em) / (2 * step)
        w = np.abs(2 * np.pi * R @ M[a])  # |d phase / d k_a| of every R
        h1, h2, h3 = (w * cn).sum(), (w**2 * cn).sum(), (w**3 * cn).sum()
        e3 = h3 + 6 * h1 * h2 / gap + 12 * h1**3 / gap**2
        bound = step**2 / 6 * e3 + 16 * EPS * emax / step
        dev = np.abs(q[a] - fd).max()
        print(f"Cartesian velocity {a}: max |<O_a> - central difference| {dev:.3e} (bound {bound:.2e}, max|v| {np.abs(fd).max():.3f})")
        assert dev <= bound and np.abs(fd).max() > 1e-2


# ---------------------------------------------------------------- 5. the restatement against a closed form
def cosine_band(npt):
    """e = -2 cos 2 pi kappa on npt points, v = de/dkappa from the derivative series through the restatement, and v^2."""
    import autobzcore.jl_amd as abz
    h = abz.FourierSeries(np.array([-1.0, 0.0, -1.0]), period=1.0, first=-1)
    so = orc.FourierSeries(h.c, period=1.0, first=h.first, ndim=1)
    do = orc.FourierSeries(h.derivative(0).c, period=1.0, first=h.first, ndim=1)
    kappa = (np.arange(npt) / npt).reshape(-1, 1)
    H, O = orc.evaluate_many(so, kappa), orc.evaluate_many(do, kappa)
    eig = np.real(xn.matrices(H))[:, 0, :]  # [npt, 1]
    A = xn.elements(H, [O], [(0, -1), (0, 0)])  # [2, npt, 1]
    assert np.abs(eig[:, 0] + 2 * np.cos(2 * np.pi * kappa[:, 0])).max() <= 1e-14
    assert np.abs(A[0, :, 0] - 4 * np.pi * np.sin(2 * np.pi * kappa[:, 0])).max() <= 1e-13
    return eig, A


def test_restatement_gives_the_transport_integral_of_a_cosine_band():
    """One band in one dimension, e = -2 cos 2 pi kappa, v = 4 pi sin 2 pi kappa: N_A(E) = int v^2 theta(E - e) dkappa =
    (4 pi)^2 [kappa_E - sin(4 pi kappa_E) / 4 pi], kappa_E = arccos(-E / 2) / 2 pi, and 8 pi^2 above the band (there the
    tetrahedron sum is the trapezoidal rule of a trigonometric polynomial: exact).  Measured on the CPU: 78.95683521 against
    78.95683520871, and at E = (-1.5, -0.7, 0, 0.3, 1.1, 1.5) deviations of at most 0.0060 (npt = 100) and 0.0010 (npt = 400);
    asserted 0.01 and 0.002."""
    Es = np.array([-1.5, -0.7, 0.0, 0.3, 1.1, 1.5])
    kE = np.arccos(-Es / 2) / (2 * np.pi)
    exact = (4 * np.pi) ** 2 * (kE - np.sin(4 * np.pi * kE) / (4 * np.pi))
    for npt, asserted in ((100, 0.01), (400, 0.002)):
        eig, A = cosine_band(npt)
        _, N = wn.wltm(eig, A[1], np.concatenate([Es, [2.5]]))
        top = abs(N[-1, 0] - 8 * np.pi**2)
        dev = np.abs(N[:-1, 0] - exact).max()
        print(f"cosine band npt={npt}: N_A above the band {N[-1, 0]:.8f} (8 pi^2 = {8 * np.pi**2:.11f}), max dev inside {dev:.4f}")
        assert top <= 1e-9 * 8 * np.pi**2 and dev <= asserted

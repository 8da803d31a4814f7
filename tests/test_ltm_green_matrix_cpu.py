"""Local Green's function matrix G_pq(z) of the tetrahedron method, CPU side: the bindings of abz_rule_ltm_projectors, and the
numpy helper of the device tests (tests/gloc_ltm_numpy.py) against an exact identity, its sum rules and a plain grid mean of the
resolvent.  The kernels are checked in test_gpu_ltm_green_matrix.py."""
import inspect
import os
import re

import numpy as np
import pytest

import abz_oracle as orc
import gloc_ltm_numpy as gl
import gltm_numpy as gn
from test_gpu_parity import rand_series

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0**-52


# ---------------------------------------------------------------- 1. bindings
def test_ltm_projectors_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert re.search(r"^int abz_rule_ltm_projectors\(abz_rule\* r, const int32_t\* pairs(?: /\*.*?\*/)?, int npairs\);", hdr, flags=re.M)
    assert "abz_rule_ltm_projectors" in L.PROTOTYPES
    assert hasattr(L.lib(), "abz_rule_ltm_projectors")
    assert ":abz_rule_ltm_projectors" in jl and "function ltm_projectors!" in jl and "function ltm_green_matrix" in jl
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_K_COUNT"] == 8 and defs["ABZ_VERSION"] == 502 and defs["ABZ_LTM_MAX_COMP"] == 16
    for cls in (abz.DeviceRule, abz.UnfoldedRule):
        assert hasattr(cls, "ltm_projectors") and hasattr(cls, "ltm_green_matrix")
    assert list(inspect.signature(abz.DeviceRule.ltm_green_matrix).parameters) == ["self", "zs", "orbitals"]
    assert list(inspect.signature(abz.dos.green_local).parameters) == ["prob_or_cache", "zs", "orbitals"]
    assert "eigen-solve" in abz.DeviceRule.ltm_green_matrix.__doc__  # each group repeats it: the docstring says so


def test_green_local_refuses_before_anything_is_built():
    """A k-sharded series is refused on the host, before a cache or a rule is made: no device is touched."""
    import autobzcore.jl_amd as abz

    class Sharded:
        kshard = (0, 2)

    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    h.device = lambda: Sharded()
    bz = abz.load_bz(abz.FBZ(), [[2 * np.pi]])
    with pytest.raises(NotImplementedError, match="k-sharded"):
        abz.dos.green_local(abz.DOSProblem(h, 0.0, bz), [0.3 + 0.1j])


# ---------------------------------------------------------------- 2. exact identity
def rotated_bands(d, npt, n=3, seed=5):
    """H(k) = Q diag(e_b(k)) Q^dagger on the npt^d grid with a fixed unitary Q and e_b = 3 b + sum_j c_bj cos(2 pi k_j),
    sum_j |c_bj| <= 1: neighbouring bands stay at least 1 apart.  -> (eig [npt]*d + [n], H [npt]*d + [n, n], Q, c [n, d])."""
    rng = np.random.default_rng(seed + d)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    coef = rng.uniform(-1.0, 1.0, (n, d)) / d
    k = np.stack(np.meshgrid(*([np.arange(npt) / npt] * d), indexing="ij"), axis=-1)  # [npt]*d + [d]
    eig = 3.0 * np.arange(n) + np.einsum("...j,bj->...b", np.cos(2 * np.pi * k), coef)
    H = np.einsum("pb,...b,qb->...pq", q, eig, q.conj())
    return eig, H, q, coef


def identity_z(eig):
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    re = np.array([lo + 0.13 * w, lo + 0.5 * w, hi - 0.2 * w, hi + 0.4 * w])
    return np.concatenate([re + 1e-8j, re - 1e-8j, re + 0.3j, re - 0.3j])


def rotated_reference(eig, q, zs):
    """Q diag(g_b(z)) Q^dagger, g_b the tetrahedron trace of band b alone."""
    g = np.stack([gn.green_trace(eig[..., b:b + 1], zs) for b in range(eig.shape[-1])], axis=1)  # [nz, n]
    return np.einsum("pb,zb,qb->zpq", q, g, q.conj())


@pytest.mark.parametrize("d,npt", [(1, 7), (2, 5), (3, 4)])
def test_rotated_bands_give_the_rotated_traces(d, npt):
    """The projector of a fixed unitary is constant over the zone, so the matrix is the rotation of the single-band traces."""
    eig, H, q, _ = rotated_bands(d, npt)
    assert np.all(np.diff(eig, axis=-1) >= 1.0 - 1e-12)
    zs = identity_z(eig)
    G = gl.green_matrix(eig, H, zs)
    ref = rotated_reference(eig, q, zs)
    dev = np.abs(G - ref).max()
    bound = 1e-12 * max(1.0, np.abs(ref).max())
    print(f"rotated bands d={d} npt={npt}: max dev {dev:.3e} (bound {bound:.1e}, max|ref| {np.abs(ref).max():.3e})")
    assert G.shape == (len(zs), 3, 3) and dev <= bound


# ---------------------------------------------------------------- 3. sum rules
def test_sum_rules_of_the_helper():
    """sum_p G_pp = tr G and G_qp(z) = conj(G_pq(conj z)) on a random Hermitian 3-band series.  The second holds to the bit (the
    restatement conjugates below the real axis).  The first holds to rounding: every simplex has sum_i W_i = J to 46 eps of
    max_i |W_i| <= 1 / eta (test_ltm_green_weighted_cpu.WORST_SUM_EPS) at each of its d + 1 corners, and sum_p P^b_pp = 1 to
    n eps, for n bands."""
    n, npt, eta = 3, 6, 0.05
    c, first = rand_series(np.random.default_rng(21), (3, 3), n, hermitian=True)
    H = np.asarray(orc.fourier_ptr(orc.FourierSeries(c, period=1.0, first=first, ndim=2), npt))
    eig = np.linalg.eigvalsh(H, UPLO="U")
    lo, hi = eig.min(), eig.max()
    zs = np.linspace(lo - 0.5, hi + 0.5, 9) + 1j * np.array([eta, -eta, 0.3] * 3)
    G = gl.green_matrix(eig, H, zs)
    tr = gn.green_trace(eig, zs)
    dev = np.abs(np.trace(G, axis1=1, axis2=2) - tr).max()
    bound = (46 * 3 + n) * EPS * n / eta
    print(f"sum_p G_pp against tr G: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound
    Gc = gl.green_matrix(eig, H, np.conj(zs))
    assert np.array_equal(np.ascontiguousarray(G.transpose(0, 2, 1)).view(np.float64), np.conj(Gc).view(np.float64))
    assert np.abs(G - G.transpose(0, 2, 1)).max() > 1e-3  # a complex Hermitian H: the matrix is not symmetric


# ---------------------------------------------------------------- 4. convergence
CONVERGENCE = 7.83e-3  # measured: max |G_LTM(npt = 16) - mean inv(z - H) (npt = 192)| over the z list below


def test_matrix_converges_to_the_grid_mean_of_the_resolvent():
    """The helper's matrix on 16^2 points against the plain grid mean of inv(z - H(k)) on 192^2 points (the oracle's series
    evaluation), 3 random Hermitian bands in 2-D (bandwidth 20.7), eta = 0.4.  The grid mean of a function analytic in a strip
    converges exponentially in npt eta / bandwidth: at 192 points it differs by 1.2e-8 from 256 points (measured on the CPU),
    so the difference is the tetrahedron method's O(1/npt^2) interpolation error.  Measured: 7.83e-3 (4.27 times the value at
    npt = 32, 1.83e-3: second order); the assertion is twice that, the margin for the choice of z."""
    n, eta = 3, 0.4
    c, first = rand_series(np.random.default_rng(21), (3, 3), n, hermitian=True)
    so = orc.FourierSeries(c, period=1.0, first=first, ndim=2)
    H = np.asarray(orc.fourier_ptr(so, 16))
    eig = np.linalg.eigvalsh(H, UPLO="U")
    zs = np.linspace(eig.min() - 0.3, eig.max() + 0.3, 7) + 1j * eta
    G = gl.green_matrix(eig, H, zs)
    Hf = np.asarray(orc.fourier_ptr(so, 192)).reshape(-1, n, n)
    ref = np.stack([np.linalg.inv(z * np.eye(n) - Hf).mean(axis=0) for z in zs])
    dev = np.abs(G - ref).max()
    print(f"LTM 16^2 against the grid mean of the resolvent on 192^2: max dev {dev:.3e} (asserted {2 * CONVERGENCE:.2e})")
    assert dev <= 2 * CONVERGENCE
    assert np.abs(ref - ref.transpose(0, 2, 1)).max() > 1e-3  # the off-diagonal elements are not trivially symmetric

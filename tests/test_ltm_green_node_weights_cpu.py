"""Complex integration weights W_b(k; z) of the Green's function per grid point and band, CPU side: the bindings of
abz_rule_ltm_green_node_weights / _ptr / _dot / _fold / _matrix, the scatter-form restatement (tests/gnodew_numpy.py) against
the restatements of the trace and of the weighted Green's function and its own identities, and what the Python mirror refuses
before it touches a device.  The device kernel is checked against the same restatement in test_gpu_ltm_green_node_weights.py.

Bounds.  The restatement scatters the very per-simplex corner weights gwltm_numpy.green_weighted contracts (the same function
on the same sorted corners: the same bits), so contractions of W differ from it by the order of summation only: a sum of N
terms x_i carries at most N eps sum |x_i| (eps = 2^-52 = 2 u: the first-order bound (N - 1) u sum |x_i| with a factor 2 to
spare), N = the nk n entries of the contraction plus the (d+1)! terms of an entry.  Where an identity of the corner weights is
used (sum_i W_i = J, sum_i x_i W_i = z J - 1) its own tested bound per simplex is added: 4 x WORST_SUM_EPS of |J| and
4 x WORST_MOMENT_EPS of |z J| + 1 (test_ltm_green_weighted_cpu.py)."""
import itertools
import math
import os
import re

import numpy as np
import pytest

import bloechl_numpy as bn
import gltm_numpy as gn
import gnodew_numpy as gnw
import gwltm_numpy as gw
import unfold_numpy as un
from test_ltm_green_weighted_cpu import WORST_MOMENT_EPS, WORST_SUM_EPS
from test_ltm_node_weights_cpu import CASES, bands

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0**-52


def z_list(eig):
    """Inside the bands at Im z = 1e-2, 1e-6, 0.5 and -1e-2, below and above them, a node's own eigenvalue at +1e-8j."""
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo if hi > lo else 1.0
    own = float(eig.reshape(-1)[(7 * eig.size) // 11])
    return np.array([lo + 0.3 * w + 1e-2j, lo + 0.55 * w + 1e-6j, lo + 0.7 * w + 0.5j, lo + 0.4 * w - 1e-2j, lo - 0.4 * w + 1e-3j,
                     hi + 0.6 * w - 0.2j, own + 1e-8j])


def nterms(eig):
    d = eig.ndim - 1
    return eig.size + math.factorial(d + 1)


# ---------------------------------------------------------------- 1. bindings
def test_green_node_weight_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    protos = {
        "abz_rule_ltm_green_node_weights": r"^int abz_rule_ltm_green_node_weights\(abz_rule\* r, const double\* z /\* \[nz\]\[2\] \*/, int nz, "
                                           r"double\* out /\* \[nz\]\[nk\]\[n\]\[2\] or NULL \*/\);",
        "abz_rule_ltm_green_node_weights_ptr": r"^int abz_rule_ltm_green_node_weights_ptr\(const abz_rule\* r, void\*\* base, int64_t\* nbytes, int\* nz\);",
        "abz_rule_ltm_green_node_weights_dot": r"^int abz_rule_ltm_green_node_weights_dot\(abz_rule\* r, double\* out /\* \[nz\]\[ncomp\]\[2\] \*/\);",
        "abz_rule_ltm_green_node_weights_fold": r"^int abz_rule_ltm_green_node_weights_fold\(abz_rule\* r, double\* out /\* \[nz\]\[nirr\]\[n\]\[2\] \*/\);",
        "abz_rule_ltm_green_node_weights_matrix": r"^int abz_rule_ltm_green_node_weights_matrix\(abz_rule\* r, double\* out /\* \[nz\]\[n\]\[n\]\[2\] \*/\);",
    }
    for name, rx in protos.items():
        assert re.search(rx, hdr, flags=re.M), name
        assert name in L.PROTOTYPES, name
        assert hasattr(L.lib(), name), name
        assert ":" + name in jl, name
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_LTM_GREEN_NODEW_MAX_Z"] == L.LTM_GREEN_NODEW_MAX_Z == 8
    assert 2 * defs["ABZ_LTM_GREEN_NODEW_MAX_Z"] <= defs["ABZ_LTM_NODEW_MAX_E"]  # 2 nz real sets fit the consumers of a real block
    assert defs["ABZ_VERSION"] == 502 and L.lib().abz_version() == 502 and defs["ABZ_K_COUNT"] == 8
    for meth in ("ltm_green_node_weights", "ltm_green_node_weights_ptr", "ltm_green_node_weights_dot", "ltm_green_node_weights_matrix"):
        assert hasattr(abz.DeviceRule, meth), meth
    assert hasattr(abz.UnfoldedRule, "ltm_green_node_weights_fold") and not hasattr(abz.DeviceRule, "ltm_green_node_weights_fold")
    assert callable(abz.dos.green_weights) and callable(abz.dos.green_local_fused)
    # a null handle is refused by every entry point before anything else is looked at
    for call in (lambda: L.lib().abz_rule_ltm_green_node_weights(None, None, 1, None),
                 lambda: L.lib().abz_rule_ltm_green_node_weights_ptr(None, None, None, None),
                 lambda: L.lib().abz_rule_ltm_green_node_weights_dot(None, None),
                 lambda: L.lib().abz_rule_ltm_green_node_weights_fold(None, None),
                 lambda: L.lib().abz_rule_ltm_green_node_weights_matrix(None, None)):
        assert call() == L.ERR_ARG and b"null rule handle" in L.lib().abz_last_error()


# ---------------------------------------------------------------- 2. identities of the restatement
@pytest.mark.parametrize("d,npt,n", CASES)
def test_contracted_weights_are_the_trace_and_the_weighted_green_function(d, npt, n):
    """sum_k sum_b W against gltm_numpy.green_trace, sum W A against gwltm_numpy.green_weighted for random A, and
    sum e W = z tr G - n."""
    eig = bands(d, npt, n)
    zs = z_list(eig)
    rng = np.random.default_rng(11)
    A = rng.standard_normal((3,) + eig.shape)
    simp = gnw.simplices(eig)
    W = gnw.node_weights_from(simp, eig.shape, zs)
    assert W.shape == (len(zs),) + eig.shape and W.dtype == np.complex128
    Wf = W.reshape(len(zs), -1)
    N = nterms(eig)
    w = 1.0 / (math.factorial(d) * npt ** d)
    t = gn.green_trace(eig, zs)
    G = gw.green_weighted(eig, A, zs)
    for i, z in enumerate(zs):
        absW = float(np.abs(Wf[i]).sum())
        J = gn.simplex_J_any(simp[0], z)
        sumJ = w * float(np.abs(J).sum())
        # the trace: the identity sum_i W_i = J per simplex, then the order of summation
        dev, bound = abs(Wf[i].sum() - t[i]), 4 * WORST_SUM_EPS * EPS * sumJ + N * EPS * (absW + sumJ)
        print(f"d={d} npt={npt} n={n} z={z}: |sum W - tr G| = {dev:.2e} (bound {bound:.1e})")
        assert dev <= bound
        # elements: the order of summation alone
        for c in range(3):
            a = A[c].reshape(-1)
            dev, bound = abs(Wf[i] @ a - G[i, c]), (N + 2) * EPS * 2 * float((np.abs(Wf[i]) * np.abs(a)).sum())
            assert dev <= bound, (z, c, dev, bound)
        # the first moment: sum_i x_i W_i = z J - 1 per simplex, and tr G itself through the first identity
        e = eig.reshape(-1)
        first = w * float((np.abs(z * J) + 1.0).sum())
        dev = abs(Wf[i] @ e - (z * t[i] - n))
        bound = (4 * WORST_MOMENT_EPS * EPS * first + (N + 2) * EPS * (float((np.abs(Wf[i]) * np.abs(e)).sum()) + first)
                 + abs(z) * (4 * WORST_SUM_EPS * EPS * sumJ + N * EPS * sumJ))
        print(f"d={d} npt={npt} n={n} z={z}: |sum e W - (z tr G - n)| = {dev:.2e} (bound {bound:.1e})")
        assert dev <= bound


@pytest.mark.parametrize("d,npt,n", CASES)
def test_conjugate_z_gives_the_conjugate_weights_to_the_bit(d, npt, n):
    eig = bands(d, npt, n, seed=2)
    zs = z_list(eig)
    simp = gnw.simplices(eig)
    W, Wc = gnw.node_weights_from(simp, eig.shape, zs), gnw.node_weights_from(simp, eig.shape, np.conj(zs))
    assert np.array_equal(Wc.view(np.float64), np.conj(W).view(np.float64))
    assert np.abs(W.imag).max() > 0.0


@pytest.mark.parametrize("d,npt", [(1, 2), (1, 5), (2, 2), (2, 4), (3, 2), (3, 3)])
def test_a_flat_band_weighs_every_node_alike(d, npt):
    """e == e0: every simplex gives each corner 1 / ((d+1) u) exactly (test_equal_and_nearly_equal_corners), so nk W is
    1 / (z - e0) up to the roundings of the (d+1)! equal terms of a node, the division by d + 1, the weight and the product with
    nk, and the one of the reference's reciprocal: (d+1)! + 6 eps of |1 / u|."""
    e0 = 0.25
    eig = np.full((npt,) * d + (1,), e0)
    zs = np.array([e0 + 1e-8j, e0 + 0.3 - 1e-2j, -4.0 + 0.5j, e0 - 1e-6j])
    W = gnw.node_weights(eig, zs)
    nk = npt ** d
    for i, z in enumerate(zs):
        ref = 1.0 / (z - e0)
        dev = float(np.abs(nk * W[i] - ref).max())
        print(f"flat band d={d} npt={npt} z={z}: |nk W - 1/(z - e0)| = {dev / (EPS * abs(ref)):.1f} eps")
        assert dev <= (math.factorial(d + 1) + 6) * EPS * abs(ref)
        assert np.all(W[i] == W[i].reshape(-1)[0])  # every node the same bits


@pytest.mark.parametrize("d,npt", [(2, 6), (3, 4)])
def test_orbit_sums_contract_like_the_full_grid(d, npt):
    """The cosine band has the whole (hyper)cubic group (made exact here as an unfolded rule makes it: copies of the values at the
    irreducible nodes); for an invariant A = f(e) the weights summed over each orbit and contracted on the irreducible nodes give
    the full-grid sum: a reordering of the same nk terms."""
    syms = [np.diag(s) @ np.eye(d, dtype=np.int64)[list(p)] for p in itertools.permutations(range(d)) for s in itertools.product((1, -1), repeat=d)]
    idx, mult = un.irreducible(npt, d, syms)
    node_of = un.orbit_map(npt, d, syms, idx / npt)
    eig = un.unfold(un.grid_flat(bn.cosine_band(npt, d=d))[un.flat_index(idx, npt)], node_of, npt, d)
    zs = z_list(eig)[:4]
    W = gnw.node_weights(eig, zs)
    Wn = W.reshape(len(zs), -1, 1)  # [nz, nk, 1] in the node order of un.unfold (i_1 fastest), as a rule exports
    en = eig.reshape(-1, 1)
    assert np.array_equal(en[un.flat_index(idx, npt)][node_of], en)  # the band is invariant: every point has its node's value
    fold = np.zeros((len(zs), len(idx), 1), dtype=np.complex128)
    np.add.at(fold, (slice(None), node_of), Wn)
    assert np.array_equal(np.bincount(node_of), mult)
    for f in (np.square, np.sin):
        full = np.einsum("zkb,kb->z", Wn, f(en))
        folded = np.einsum("zjb,jb->z", fold, f(en[un.flat_index(idx, npt)]))
        bound = nterms(eig) * EPS * 2 * float((np.abs(Wn) * np.abs(f(en))[None]).sum(axis=(1, 2)).max())
        dev = float(np.abs(full - folded).max())
        print(f"d={d} fold of {f.__name__}(e): |folded - full| = {dev:.2e} (bound {bound:.1e})")
        assert dev <= bound
    # the mesh has fewer symmetries than the band: a fold is a sum over the orbit, not multiplicity x weight
    rep = un.flat_index(idx, npt)
    assert np.abs(fold - mult[None, :, None] * Wn[:, rep]).max() * npt ** d > 1e-3


# ---------------------------------------------------------------- 3. what the Python mirror refuses without a device
def test_mirror_argument_errors():
    import autobzcore.jl_amd as abz
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    prob = abz.DOSProblem(h, 0.0, abz.load_bz(abz.FBZ(), [[2 * np.pi]]))
    zs9 = 0.1 * np.arange(9) + 0.2j
    for bad, match in ((zs9, "1..8"), ([], "1..8"), ([0.3 + 0.1j, 0.4], "real"), (0.5, "real"), ([0.1 + 1j * np.nan], "not finite"),
                       ([np.inf + 0.1j], "not finite")):
        with pytest.raises(ValueError, match=match):
            abz.dos.green_weights(prob, bad)
    rule = object.__new__(abz.DeviceRule)
    rule.shard, rule._ltm_halo = None, False
    for bad, match in ((zs9, "1..8"), ([], "1..8"), ([0.4], "real"), ([1j * np.inf], "not finite")):
        with pytest.raises(ValueError, match=match):
            rule.ltm_green_node_weights(bad)
    with pytest.raises(ValueError, match="attached"):
        rule.ltm_green_node_weights_dot(elements="energy")
    # fold=True needs a symmetric cache of a symmetric zone; the fused matrix needs a cache that is not one.  (Caches without a
    # rule: abz.dos.init would build one on the device, and both refusals come before the rule is looked at.)
    plain = abz.dos.DOSCache(prob.H, prob.domain, prob.p, abz.LTM(npt=8), None, {})
    with pytest.raises(ValueError, match="fold=True"):
        abz.dos.green_weights(plain, 0.3 + 0.1j, fold=True)
    c3 = np.zeros((3, 3, 3, 1, 1))
    c3[0, 1, 1] = c3[2, 1, 1] = c3[1, 0, 1] = c3[1, 2, 1] = c3[1, 1, 0] = c3[1, 1, 2] = 0.5
    s3 = abz.FourierSeries(c3, period=1.0, offset=-2)
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sprob = abz.DOSProblem(s3, 0.0, cub)
    sym = abz.dos.DOSCache(sprob.H, sprob.domain, sprob.p, abz.LTM(npt=4, symmetric=True), None, {})
    with pytest.raises(ValueError, match="symmetric=False"):
        abz.dos.green_local_fused(sym, [0.3 + 0.1j])
    with pytest.raises(ValueError, match="fold=True"):  # a symmetric algorithm on a zone without symmetries
        abz.dos.green_weights(abz.dos.DOSCache(prob.H, prob.domain, prob.p, abz.LTM(npt=8, symmetric=True), None, {}), 0.3 + 0.1j, fold=True)
    with pytest.raises(ValueError, match="LTM cache"):
        abz.dos.green_weights(abz.dos.DOSCache(prob.H, prob.domain, prob.p, abz.GGR(npt=8), None, {}), 0.3 + 0.1j)
    # a k-sharded series is refused before anything is built
    class Sharded:
        kshard = (0, 2)

    h.device = lambda: Sharded()
    with pytest.raises(NotImplementedError, match="k-sharded"):
        abz.dos.green_weights(abz.DOSProblem(h, 0.0, abz.load_bz(abz.FBZ(), [[2 * np.pi]])), 0.3 + 0.1j)
    with pytest.raises(NotImplementedError, match="k-sharded"):
        abz.dos.green_local_fused(abz.DOSProblem(h, 0.0, abz.load_bz(abz.FBZ(), [[2 * np.pi]])), [0.3 + 0.1j])
    rule.shard = (0, 2)
    for call in (lambda: rule.ltm_green_node_weights([0.1j]), rule.ltm_green_node_weights_ptr, rule.ltm_green_node_weights_dot,
                 rule.ltm_green_node_weights_matrix):
        with pytest.raises(NotImplementedError, match="halo"):
            call()


def test_green_node_weights_fail_loudly_without_gpu():
    import torch
    import autobzcore.jl_amd as abz
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    prob = abz.DOSProblem(h, 0.0, abz.load_bz(abz.FBZ(), [[2 * np.pi]]))
    for call in (lambda: abz.dos.green_weights(prob, [0.1 + 0.2j]),
                 lambda: abz.dos.green_local_fused(prob, [0.1 + 0.2j]),
                 lambda: h.device().rule(8, None, abz._lib.WANT_EIG).ltm_green_node_weights([0.1j]),
                 lambda: h.device().rule(8, None, abz._lib.WANT_EIG).ltm_green_node_weights_ptr()):
        with pytest.raises(abz.AbzError, match=rf"libabzhip error {abz._lib.ERR_NOGPU}\b"):  # ABZ_ERR_NOGPU: no CPU fallback
            call()

"""Integration weights per grid point and band, CPU side: the scatter-form restatement (tests/nodew_numpy.py) against the
restatements of the weighted tetrahedron method and of the curvature correction, its own sum rules and the symmetry of the Kuhn
mesh; and the bindings of abz_rule_ltm_node_weights / _ptr / _dot / _fold.  The device kernels are checked against the same
restatement in test_gpu_ltm_node_weights.py."""
import itertools
import os
import re

import numpy as np
import pytest

import bloechl_numpy as bn
import nodew_numpy as nw
import wltm_numpy as wn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(d, npt, n) for d in (1, 2, 3) for npt, n in ((2, 1), (4, 2), (5, 3), (7, 1))]


def bands(d, npt, n, seed=0):
    """Smooth periodic bands plus noise, sorted ascending at every node: [npt]*d + [n]"""
    rng = np.random.default_rng(seed + 100 * d + npt)
    k = 2.0 * np.pi * np.arange(npt) / npt
    ks = np.meshgrid(*([k] * d), indexing="ij")
    e = np.stack([sum(np.cos(ks[j] + 0.3 * b) * (1.0 + 0.2 * j) for j in range(d)) + 0.7 * b for b in range(n)], axis=-1)
    return np.sort(e + 0.05 * rng.standard_normal(e.shape), axis=-1)


def energies(eig, rng):
    lo, hi = float(eig.min()), float(eig.max())
    flat = eig.reshape(-1)
    return np.concatenate([[lo - 0.5, hi + 0.5, lo, hi, flat[len(flat) // 2], flat[1 % len(flat)]], lo + (hi - lo) * rng.random(5)])


def bound(ref):
    return 1e-12 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("d,npt,n", CASES)
def test_contracted_weights_are_the_weighted_method(d, npt, n):
    """einsum(W, A) against wltm_numpy's g_A and N_A and against N_A + bloechl_numpy.correction, for random A."""
    eig = bands(d, npt, n)
    rng = np.random.default_rng(7)
    Es = energies(eig, rng)
    A = rng.standard_normal((3,) + eig.shape)
    g_ref, N_ref = wn.wltm(eig, A, Es)
    C_ref = N_ref + bn.correction(eig, A, Es)
    simp = nw.simplices(eig)
    for kind, ref in (("dos", g_ref), ("states", N_ref), ("corrected", C_ref)):
        W = nw.node_weights_from(simp, eig.shape, Es, kind)
        assert W.shape == (len(Es),) + eig.shape
        u = W.reshape(len(Es), -1) @ A.reshape(3, -1).T  # einsum(W, A) over (k, b)
        dev = np.abs(u - ref).max()
        print(f"d={d} npt={npt} n={n} {kind}: einsum(W, A) - ref {dev:.2e} (bound {bound(ref):.1e})")
        assert dev <= bound(ref), (kind, dev)


@pytest.mark.parametrize("d,npt,n", CASES)
def test_sum_rules(d, npt, n):
    eig = bands(d, npt, n, seed=3)
    lo, hi = float(eig.min()), float(eig.max())
    nk = npt ** d
    for kind in nw.KINDS:
        W = nw.node_weights(eig, [lo - 1.0, hi + 1.0, np.nextafter(lo, -np.inf), hi], kind)
        assert np.all(W[0] == 0.0) and np.all(W[2] == 0.0)  # nothing below the bands
        if kind == "dos":
            assert np.all(W[1] == 0.0) and np.all(W[3] == 0.0)
        else:  # every node of a full band weighs 1 / nk: sum = n
            assert np.abs(nk * W[1] - 1.0).max() <= 1e-14 and np.abs(nk * W[3] - 1.0).max() <= 1e-14
            assert abs(W[1].sum() - n) <= 1e-13 * n
    # inside the bands: the states sum to N(E), the correction block to 0 (kappa_T = 0 for A = 1)
    Es = lo + (hi - lo) * np.array([0.2, 0.5, 0.8])
    _, N = wn.wltm(eig, np.ones_like(eig), Es)
    S = nw.node_weights(eig, Es, "states")
    C = nw.node_weights(eig, Es, "corrected")
    assert np.abs(S.reshape(3, -1).sum(axis=1) - N[:, 0]).max() <= bound(N)
    assert np.abs((C - S).reshape(3, -1).sum(axis=1)).max() <= 1e-13 * n
    assert np.all(S >= -1e-16) and np.all(nk * S <= 1.0 + 1e-12)


@pytest.mark.parametrize("d", [2, 3])
def test_weights_of_a_cosine_band_have_the_symmetry_of_the_kuhn_mesh(d):
    """The band -2 sum_j cos k_j is invariant under all 2^d d! operations of the (hyper)cube; the Kuhn split only under the d!
    permutations of the axes times the inversion k -> -k (12 of 48 in 3-D, 4 of 8 in 2-D).  The weights follow the mesh: invariant
    under those, and NOT under a single mirror -- which is why a fold over orbits is a sum, not multiplicity x weight."""
    npt = 6
    eig = bn.cosine_band(npt, d=d)
    Es = np.array([-1.3, 0.4, 1.7])
    for kind in nw.KINDS:
        W = nw.node_weights(eig, Es, kind)[..., 0]  # [nE] + [npt]*d
        scale = max(1.0, float(np.abs(W).max() * npt ** d))
        for perm in itertools.permutations(range(d)):
            for inv in (False, True):
                V = np.transpose(W, (0,) + tuple(1 + p for p in perm))
                if inv:
                    for ax in range(1, d + 1):
                        V = np.roll(np.flip(V, axis=ax), 1, axis=ax)  # index i -> -i mod npt
                dev = np.abs(V - W).max() * npt ** d
                assert dev <= 1e-12 * scale, (kind, perm, inv, dev)
        mirror = np.roll(np.flip(W, axis=1), 1, axis=1)  # k_1 -> -k_1 alone
        dev = np.abs(mirror - W).max() * npt ** d
        print(f"d={d} {kind}: nk max|w(mirror k) - w(k)| = {dev:.3e}")
        assert dev > 1e-3, (kind, dev)


def test_node_weight_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    protos = {
        "abz_rule_ltm_node_weights": r"^int abz_rule_ltm_node_weights\(abz_rule\* r, const double\* E, int nE, int what, double\* out /\* \[nE\]\[nk\]\[n\] or NULL \*/\);",
        "abz_rule_ltm_node_weights_ptr": r"^int abz_rule_ltm_node_weights_ptr\(const abz_rule\* r, void\*\* base, int64_t\* nbytes, int\* nE\);",
        "abz_rule_ltm_node_weights_dot": r"^int abz_rule_ltm_node_weights_dot\(abz_rule\* r, double\* out /\* \[nE\]\[ncomp\] \*/\);",
        "abz_rule_ltm_node_weights_fold": r"^int abz_rule_ltm_node_weights_fold\(abz_rule\* r, double\* out /\* \[nE\]\[nirr\]\[n\] \*/\);",
    }
    for name, rx in protos.items():
        assert re.search(rx, hdr, flags=re.M), name
        assert name in L.PROTOTYPES, name
        assert hasattr(L.lib(), name), name
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_LTM_NODEW_MAX_E"] == L.LTM_NODEW_MAX_E == 16
    assert defs["ABZ_VERSION"] == 502 and L.lib().abz_version() == 502
    for meth in ("ltm_node_weights", "ltm_node_weights_dot", "ltm_node_weights_ptr"):
        assert hasattr(abz.DeviceRule, meth), meth
    assert hasattr(abz.series.UnfoldedRule, "ltm_node_weights_fold") and not hasattr(abz.DeviceRule, "ltm_node_weights_fold")
    assert callable(abz.dos.integration_weights)
    # a null handle is refused by every entry point before anything else is looked at
    for call in (lambda: L.lib().abz_rule_ltm_node_weights(None, None, 1, L.LTM_STATES, None),
                 lambda: L.lib().abz_rule_ltm_node_weights_ptr(None, None, None, None),
                 lambda: L.lib().abz_rule_ltm_node_weights_dot(None, None),
                 lambda: L.lib().abz_rule_ltm_node_weights_fold(None, None)):
        assert call() == L.ERR_ARG and b"null rule handle" in L.lib().abz_last_error()


def test_mirror_argument_errors():
    """What the Python mirror refuses before it touches a device."""
    import autobzcore.jl_amd as abz
    prob = abz.DOSProblem(abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2), 0.0,
                          abz.load_bz(abz.FBZ(), [[2 * np.pi]]))
    with pytest.raises(ValueError, match="exactly one"):
        abz.dos.integration_weights(prob)
    with pytest.raises(ValueError, match="exactly one"):
        abz.dos.integration_weights(prob, E=0.1, nstates=0.5)
    with pytest.raises(ValueError, match="kind"):
        abz.dos.integration_weights(prob, E=0.1, kind="bands")
    with pytest.raises(ValueError, match="correction"):
        abz.dos.integration_weights(prob, E=0.1, kind="dos", correction=True)
    # the rule's methods, on an object that has no handle to reach
    rule = object.__new__(abz.DeviceRule)
    rule.shard, rule._ltm_halo = None, False
    with pytest.raises(ValueError, match="states=True"):
        rule.ltm_node_weights([0.1], states=False, correction=True)
    with pytest.raises(ValueError, match="1..16"):
        rule.ltm_node_weights(np.zeros(17))
    with pytest.raises(ValueError, match="1..16"):
        rule.ltm_node_weights([])
    with pytest.raises(ValueError, match="attached"):
        rule.ltm_node_weights_dot(elements="energy")
    rule.shard = (0, 2)
    for call in (lambda: rule.ltm_node_weights([0.1]), rule.ltm_node_weights_ptr, rule.ltm_node_weights_dot):
        with pytest.raises(NotImplementedError, match="halo"):
            call()
    rule._ltm_halo = True
    with pytest.raises(NotImplementedError, match="ltm_node_weights on a k-sharded"):
        rule.ltm_node_weights([0.1])


def test_node_weights_fail_loudly_without_gpu():
    import torch
    import autobzcore.jl_amd as abz
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    prob = abz.DOSProblem(h, 0.0, abz.load_bz(abz.FBZ(), [[2 * np.pi]]))
    for call in (lambda: abz.dos.integration_weights(prob, E=[0.1, 0.2]),
                 lambda: abz.dos.integration_weights(prob, nstates=0.5),
                 lambda: h.device().rule(8, None, abz._lib.WANT_EIG).ltm_node_weights([0.1]),
                 lambda: h.device().rule(8, None, abz._lib.WANT_EIG).ltm_node_weights_dot(),
                 lambda: h.device().rule(8, None, abz._lib.WANT_EIG).ltm_node_weights_ptr()):
        with pytest.raises(abz.AbzError, match=rf"libabzhip error {abz._lib.ERR_NOGPU}\b"):  # ABZ_ERR_NOGPU: no CPU fallback
            call()

"""Orbital weights for the tetrahedron method, CPU side: the bindings of abz_rule_ltm_orbitals and
abz_rule_ltm_elements_export, the `eigenvectors` / `orbitals` keywords of LTM, and the numpy helper of the device tests
(tests/orbw_numpy.py).  The kernels are checked in test_gpu_ltm_orbitals.py."""
import os
import re

import numpy as np
import pytest

import abz_oracle as orc
import orbw_numpy as ow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ltm_orbitals_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    assert re.search(r"^int abz_rule_ltm_orbitals\(abz_rule\* r, const int32_t\* orb, int norb\);", hdr, flags=re.M)
    assert re.search(r"^int abz_rule_ltm_elements_export\(abz_rule\* r, int\* ncomp, double\* A\);", hdr, flags=re.M)
    for name in ("abz_rule_ltm_orbitals", "abz_rule_ltm_elements_export"):
        assert name in L.PROTOTYPES
        assert hasattr(L.lib(), name)
        assert ":" + name in jl
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_K_COUNT"] == 8 and defs["ABZ_VERSION"] == 502 and defs["ABZ_LTM_MAX_COMP"] == 16
    for cls in (abz.DeviceRule, abz.UnfoldedRule):
        assert hasattr(cls, "ltm_orbitals") and hasattr(cls, "ltm_elements_export")


def test_ltm_eigenvectors_keywords():
    import autobzcore.jl_amd as abz
    alg = abz.LTM(elements="orbitals")
    assert alg.eigenvectors == "host" and alg.orbitals is None
    assert abz.LTM().eigenvectors == "host"
    alg = abz.LTM(npt=12, elements="orbitals", eigenvectors="device")
    assert alg.eigenvectors == "device" and alg.orbitals is None and alg.npt == 12
    alg = abz.LTM(elements="orbitals", eigenvectors="device", orbitals=[2, 0, 2])
    assert alg.orbitals == (2, 0, 2)
    assert abz.LTM(elements="orbitals", eigenvectors="device", orbitals=np.array([1])).orbitals == (1,)
    for bad in ("gpu", "Device", None, 1):
        with pytest.raises(ValueError, match="eigenvectors"):
            abz.LTM(elements="orbitals", eigenvectors=bad)
    for elements in (None, "energy", lambda x, e: e[None]):
        with pytest.raises(ValueError, match="orbitals"):
            abz.LTM(elements=elements, eigenvectors="device")
    # a selection belongs to the device route
    with pytest.raises(ValueError, match="orbitals"):
        abz.LTM(elements="orbitals", orbitals=[0])
    with pytest.raises(ValueError, match="orbitals"):
        abz.LTM(elements="energy", orbitals=[0])
    for bad in ([], [0.5], "ab"):
        with pytest.raises(ValueError, match="orbitals"):
            abz.LTM(elements="orbitals", eigenvectors="device", orbitals=bad)
    # symmetric=True stays refused where the cache is made, for either route
    so = orc.tb_integer(3)
    s = abz.FourierSeries(so.c, period=1.0, first=so.first, ndim=3)
    bz = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    for ev in ("host", "device"):
        with pytest.raises(ValueError, match="orbitals"):
            abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=8, elements="orbitals", symmetric=True, eigenvectors=ev))


def test_weights_are_normalised_and_ordered():
    rng = np.random.default_rng(3)
    H = rng.standard_normal((5, 6, 6)) + 1j * rng.standard_normal((5, 6, 6))
    H = H + H.conj().transpose(0, 2, 1)
    W = ow.weights(H)
    assert W.shape == (6, 5, 6)
    assert np.abs(W.sum(axis=0) - 1.0).max() <= 1e-14 and np.abs(W.sum(axis=2) - 1.0).max() <= 1e-14
    # only the upper triangle counts
    assert np.array_equal(ow.weights(np.triu(H)), W)
    # a diagonal matrix with descending entries: band b is orbital n - 1 - b
    D = np.diag(np.arange(4.0, 0.0, -1.0))[None]
    assert np.array_equal(ow.weights(D)[:, 0, :], np.eye(4)[::-1])
    assert np.array_equal(ow.weights(np.array([1.0, 2.0])), np.ones((1, 2, 1)))


def test_cluster_sums_are_the_projector_diagonal():
    """H = Q diag(levels, each `mult` times) Q^H: the weights numpy returns inside a level are those of an arbitrary basis, their
    sum over the level is diag(P) of the level's spectral projector P = Q_level Q_level^H."""
    rng = np.random.default_rng(11)
    levels, mult = np.array([-1.5, 0.25, 0.25 + 3e-9, 2.0]), 3  # two levels closer than tol: one cluster of 6
    n = len(levels) * mult
    q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    lam = np.repeat(levels, mult)
    H = (q * lam) @ q.conj().T
    H = 0.5 * (H + H.conj().T)
    e = np.linalg.eigvalsh(H)[None]
    W = ow.weights(H[None])
    assert ow.clusters(e[0], 1e-6) == [(0, 3), (3, 9), (9, 12)]
    S = ow.cluster_sums(e, W, 1e-6)
    for a, b in ow.clusters(e[0], 1e-6):
        P = q[:, a:b] @ q[:, a:b].conj().T
        for band in range(a, b):
            assert np.abs(S[:, 0, band] - np.diag(P).real).max() <= 1e-12
    # tol = 0 links nothing: the sums are the weights themselves
    assert np.array_equal(ow.cluster_sums(e, W, 0.0), W)
    # summed over the orbitals: the dimension of the level
    assert np.abs(S.sum(axis=0) / np.array([3, 3, 3, 6, 6, 6, 6, 6, 6, 3, 3, 3]) - 1.0).max() <= 1e-12

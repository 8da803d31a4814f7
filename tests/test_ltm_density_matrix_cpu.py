"""Density matrix of the tetrahedron method in the orbital basis, CPU side: the binding of abz_rule_ltm_density_matrix, what the
Python mirrors refuse before they touch a device, the identities of the restatement tests/densmat_numpy.py, and the exact case of
a fixed unitary.  The device kernels are checked against the same restatement in test_gpu_ltm_density_matrix.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import densmat_numpy as dm
import gloc_ltm_numpy as gl
import ltm_numpy as ln
import nodew_numpy as nw
from test_ltm_green_matrix_cpu import rotated_bands

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KINDS = ("states", "corrected", "dos")


def smooth_hermitian(rng, d, npt, n):
    """A random smooth Hermitian H(k) on the npt^d grid: a constant plus one cosine and one sine term per axis, [npt]*d + [n, n]"""
    grids = np.meshgrid(*[np.arange(npt) / npt] * d, indexing="ij")

    def rh():
        a = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
        return a + a.conj().T

    H = np.zeros(tuple([npt] * d) + (n, n), complex) + rh()
    for ax in range(d):
        even = np.cos(2 * np.pi * grids[ax])[..., None, None] * rh()
        anti = rng.normal(size=(n, n))
        H = H + even + np.sin(2 * np.pi * grids[ax])[..., None, None] * 1j * (anti - anti.T)
    return H


HELPER_CASES = [(1, 8, 3), (2, 5, 4), (3, 4, 5)]


def helper_hamiltonians():
    """The H(k) of HELPER_CASES, drawn one after the other from one generator"""
    rng = np.random.default_rng(3)
    return {case: smooth_hermitian(rng, *case) for case in HELPER_CASES}


def test_density_matrix_binding():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    rx = r"^int abz_rule_ltm_density_matrix\(abz_rule\* r, double\* out /\* \[nE\]\[n\]\[n\]\[2\] \*/\);"
    assert re.search(rx, hdr, flags=re.M)
    assert L.PROTOTYPES["abz_rule_ltm_density_matrix"] == (C.c_int, [C.c_void_p, L.c_f64p])
    fn = L.lib().abz_rule_ltm_density_matrix
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, L.c_f64p]
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_VERSION"] == 502 and L.lib().abz_version() == 502
    assert hasattr(abz.DeviceRule, "ltm_density_matrix") and callable(abz.dos.density_matrix)
    # a null handle is refused before anything else is looked at
    assert fn(None, None) == L.ERR_ARG and b"null rule handle" in L.lib().abz_last_error()


def test_mirror_argument_errors():
    """What the Python mirrors refuse before they touch a device."""
    import autobzcore.jl_amd as abz
    c = np.zeros((3, 2, 2), dtype=np.complex128)
    c[1] = [[0.3, 1.0], [1.0, -0.3]]
    c[2] = [[0.1, 0.5], [0.0, -0.15]]
    c[0] = c[2].conj().T
    prob = abz.DOSProblem(abz.FourierSeries(c, period=1.0, first=(-1,), ndim=1), 0.0, abz.load_bz(abz.FBZ(), [[2 * np.pi]]))
    with pytest.raises(ValueError, match="exactly one"):
        abz.dos.density_matrix(prob)
    with pytest.raises(ValueError, match="exactly one"):
        abz.dos.density_matrix(prob, E=0.1, nstates=0.5)
    with pytest.raises(ValueError, match="kind"):
        abz.dos.density_matrix(prob, E=0.1, kind="bands")
    with pytest.raises(ValueError, match="correction"):
        abz.dos.density_matrix(prob, E=0.1, kind="dos", correction=True)
    for bad, words in (([], "not a sequence"), ([0.5, 1.0], "not a sequence"), ([0, 0], "twice"), ([0, 2], "outside 0..1"), ([-1], "outside 0..1")):
        with pytest.raises(ValueError, match=words):
            abz.dos.density_matrix(prob, E=0.1, orbitals=bad)
    # the rule's method, on an object that has no handle to reach
    rule = object.__new__(abz.DeviceRule)
    rule.shard, rule._ltm_halo = (0, 2), False
    with pytest.raises(NotImplementedError, match="halo"):
        rule.ltm_density_matrix([0.1])
    rule._ltm_halo = True
    with pytest.raises(NotImplementedError, match="ltm_density_matrix on a k-sharded"):
        rule.ltm_density_matrix()


def test_density_matrix_fails_loudly_without_gpu():
    import torch
    import autobzcore.jl_amd as abz
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = abz.FourierSeries(np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    prob = abz.DOSProblem(h, 0.0, abz.load_bz(abz.FBZ(), [[2 * np.pi]]))
    for call in (lambda: abz.dos.density_matrix(prob, E=[0.1, 0.2]),
                 lambda: abz.dos.density_matrix(prob, nstates=0.5),
                 lambda: h.device().rule(8, None, abz._lib.WANT_EIG).ltm_density_matrix([0.1])):
        with pytest.raises(abz.AbzError, match=rf"libabzhip error {abz._lib.ERR_NOGPU}\b"):  # ABZ_ERR_NOGPU: no CPU fallback
            call()


@pytest.mark.parametrize("d,npt,n", HELPER_CASES)
def test_identities_of_the_helper(d, npt, n):
    """Hermitian to the bit, tr rho = sum W, exactly 0 below the bands, I above them (0 for the DOS weights); the corrected
    weights go negative."""
    H = helper_hamiltonians()[(d, npt, n)]
    e = np.linalg.eigh(H)[0]
    Es = [e.min() - 1, np.median(e), e.flat[7], e.max() + 1]
    for kind in KINDS:
        W = nw.node_weights(e, Es, kind)
        rho = dm.density_matrix(e, H, Es, kind)
        assert rho.shape == (len(Es), n, n) and rho.dtype == np.complex128
        assert np.array_equal(rho, rho.conj().transpose(0, 2, 1)) and np.all(np.diagonal(rho, axis1=1, axis2=2).imag == 0.0)
        tr = np.trace(rho, axis1=1, axis2=2).real
        dev_tr = np.abs(tr - W.reshape(len(Es), -1).sum(axis=1)).max()
        dev_top = np.abs(rho[-1] - (np.eye(n) if kind != "dos" else 0.0)).max()
        print(f"d={d} n={n} {kind}: |tr rho - sum W| {dev_tr:.2e} (bound 1.4e-15), |rho - I| above {dev_top:.2e} (bound 4.5e-16), min w {W.min():.3e}")
        assert dev_tr <= 1.4e-15
        assert np.all(rho[0] == 0.0)
        assert dev_top <= (4.5e-16 if kind != "dos" else 0.0)
        if kind == "corrected":
            assert W.min() < 0.0  # nothing may assume w >= 0
    # a given projector tensor instead of H: the same numbers
    P = gl.projector_tensor(H)
    assert np.array_equal(dm.density_matrix(e, P, Es, "states"), dm.density_matrix(e, H, Es, "states"))
    sub = dm.density_matrix(e, P[:2, :2], Es, "states")
    assert sub.shape == (len(Es), 2, 2) and np.abs(sub - dm.density_matrix(e, H, Es, "states")[:, :2, :2]).max() <= 1e-15


@pytest.mark.parametrize("d,npt", [(1, 7), (2, 5), (3, 4)])
def test_rotated_bands_give_the_rotated_counts(d, npt):
    """H = Q diag(e_b(k)) Q^dagger with a fixed unitary and cosine bands 3 apart: the projectors are constant over the zone, so
    rho = Q diag(N_b(E)) Q^dagger with N_b the single-band count of ltm_numpy."""
    eig, H, q, _ = rotated_bands(d, npt)
    n = eig.shape[-1]
    lo, hi = float(eig.min()), float(eig.max())
    Es = np.concatenate([[lo - 0.5, hi + 0.5, float(eig[..., 1].mean())], lo + (hi - lo) * np.random.default_rng(11).random(5)])
    Nb = np.stack([ln.ltm(eig[..., b:b + 1], Es)[1] for b in range(n)], axis=1)  # [nE, n]
    ref = np.einsum("pb,eb,qb->epq", q, Nb, q.conj())
    rho = dm.density_matrix(eig, H, Es, "states")
    dev, bound = np.abs(rho - ref).max(), 1e-12 * max(1.0, np.abs(ref).max())
    print(f"rotated bands d={d} npt={npt}: max dev {dev:.3e} (bound {bound:.1e})")
    assert rho.shape == (len(Es), n, n) and dev <= bound

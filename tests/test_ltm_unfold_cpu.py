"""Tetrahedron DOS from irreducible nodes, CPU side: the bindings of abz_rule_ltm_unfold, the `symmetric` switch of LTM,
the numpy orbit map (tests/unfold_numpy.py) against the library's symptr_rule, and the restatement on numpy-unfolded
eigenvalues against the restatement on the plain grid.  The device kernels are checked in test_gpu_ltm_unfold.py."""
import os
import re

import numpy as np
import pytest

import abz_oracle as orc
import ltm_numpy as ln
import unfold_numpy as un
from test_ltm_cpu import MODELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sym_sets(abz, d):
    return {"inversion": abz.load_bz(abz.InversionSymIBZ(), np.eye(d)).syms, "cubic": abz.load_bz(abz.CubicSymIBZ(), np.eye(d)).syms}


def model_sym_sets(abz, name, d):
    """The symmetry sets a model HAS.  InversionSymIBZ is the group of the 2^d sign flips (src/brillouin.jl:248-270), mirrors
    included; graphene in its oblique lattice basis has none of the single-axis mirrors (its eigenvalues move by 1.6 under
    k_1 -> -k_1), only the inversion proper, {1, -1}."""
    if name == "graphene":
        return {"inversion": [np.eye(2, dtype=np.int64), -np.eye(2, dtype=np.int64)]}
    return sym_sets(abz, d)


def test_ltm_unfold_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    name = "abz_rule_ltm_unfold"
    assert re.search(r"^int abz_rule_ltm_unfold\(abz_rule\* src, const int32_t\* syms, int nsyms, abz_rule\*\* out\);", hdr, flags=re.M)
    assert name in L.PROTOTYPES
    assert hasattr(L.lib(), name)
    assert ":" + name in jl
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_K_COUNT"] == 8 and defs["ABZ_VERSION"] == 502
    assert hasattr(abz.DeviceRule, "unfold") and issubclass(abz.UnfoldedRule, abz.DeviceRule)
    for meth in ("ltm", "ltm_elements", "ltm_fermi", "export", "close"):
        assert hasattr(abz.UnfoldedRule, meth), meth


def test_ltm_symmetric_switch():
    import autobzcore.jl_amd as abz
    alg = abz.LTM()
    assert alg.symmetric is False and alg.npt == 50 and alg.cumulative is False and alg.elements is None
    assert abz.LTM(symmetric=True).symmetric is True
    assert abz.LTM(npt=8, elements="energy", symmetric=True).elements == "energy"
    # orbital weights are not invariant under the zone's symmetries: refused where the cache is made, before any device work
    so = orc.tb_integer(3)
    s = abz.FourierSeries(so.c, period=1.0, first=so.first, ndim=3)
    bz = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    with pytest.raises(ValueError, match="orbitals"):
        abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=8, elements="orbitals", symmetric=True))


@pytest.mark.parametrize("d,npt", [(1, 17), (1, 16), (2, 9), (2, 12), (3, 6), (3, 7)])
def test_orbits_match_symptr_rule(d, npt):
    import autobzcore.jl_amd as abz
    for label, syms in sym_sets(abz, d).items():
        idx, w = abz.symptr_rule(npt, d, syms)
        idx_np, w_np = un.irreducible(npt, d, syms)
        assert len(w_np) == len(w), (label, d, npt)
        assert np.array_equal(w_np, w) and np.array_equal(idx_np, idx), (label, d, npt)
        assert w.sum() == npt ** d
        # the map through the exported coordinates: every point lands on the node of its orbit, orbit sizes are the weights
        node_of = un.orbit_map(npt, d, syms, idx / npt)
        assert np.array_equal(np.bincount(node_of, minlength=len(w)), w), (label, d, npt)
        assert np.array_equal(node_of[un.flat_index(idx, npt)], np.arange(len(w)))
        # another representative of every orbit serves as well
        img = un.images(npt, d, syms)
        other = un.grid_points(npt, d)[img[-1][un.flat_index(idx, npt)]]
        assert np.array_equal(np.bincount(un.orbit_map(npt, d, syms, other / npt), minlength=len(w)), w)
    with pytest.raises(ValueError, match="no node"):
        un.orbit_map(npt, d, syms, idx[:-1] / npt)


@pytest.mark.parametrize("name,npt", [("int1", 48), ("int2", 12), ("graphene", 10), ("int3", 6)])
def test_restatement_on_unfolded_eigenvalues(name, npt):
    """ln.ltm on eigenvalues gathered from the irreducible nodes against ln.ltm on the plain grid, bound 1e-9 max(1, max|ref|)
    (the project's parity bound; numpy's eigenvalues at symmetry-related nodes differ in the last digits at most)."""
    import autobzcore.jl_amd as abz
    so = MODELS[name][0]()
    d = so.d
    eig = ln.grid_eigenvalues(so, npt)
    flat = un.grid_flat(eig)
    plain = flat.reshape((npt,) * d + (flat.shape[-1],))
    lo, hi = float(eig.min()), float(eig.max())
    Es = np.linspace(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), 41) + 1e-3 / 7  # off the exact corner eigenvalues
    g_ref, N_ref = ln.ltm(plain, Es)
    for label, syms in model_sym_sets(abz, name, d).items():
        idx, w = un.irreducible(npt, d, syms)
        node_of = un.orbit_map(npt, d, syms, idx / npt)
        unfolded = un.unfold(flat[un.flat_index(idx, npt)], node_of, npt, d)
        de = np.abs(unfolded - plain).max()
        g, N = ln.ltm(unfolded, Es)
        dg, dN = np.abs(g - g_ref).max(), np.abs(N - N_ref).max()
        print(f"{name} npt={npt} {label}: {len(w)} of {npt ** d} nodes, eigenvalues moved {de:.2e}, g {dg:.2e}, N {dN:.2e}")
        assert de <= 1e-9 * max(1.0, abs(lo), abs(hi))
        assert dg <= 1e-9 * max(1.0, np.abs(g_ref).max()) and dN <= 1e-9 * max(1.0, np.abs(N_ref).max())


def test_symmetrised_synthetic_series_is_cubic():
    """symmetrise() turns synthetic_wannier, which has no symmetry, into a Hermitian series with H(S k) = H(k)."""
    import autobzcore.jl_amd as abz
    so = orc.synthetic_wannier(6, rmax=2, seed=7)
    sym = un.symmetrise(so)
    c = sym.c
    assert np.abs(c - np.conj(np.flip(c, (0, 1, 2)).transpose(0, 1, 2, 4, 3))).max() <= 1e-15  # c(-R) = c(R)^dagger
    npt = 6
    H = np.asarray(orc.fourier_ptr(sym, npt))
    flatH = np.ascontiguousarray(H.transpose(2, 1, 0, 3, 4)).reshape(-1, 6, 6)
    img = un.images(npt, 3, sym_sets(abz, 3)["cubic"])
    dev = max(np.abs(flatH[row] - flatH).max() for row in img)
    assert dev <= 1e-13, dev
    H0 = np.asarray(orc.fourier_ptr(so, npt))
    flat0 = np.ascontiguousarray(H0.transpose(2, 1, 0, 3, 4)).reshape(-1, 6, 6)
    assert max(np.abs(flat0[row] - flat0).max() for row in img) > 1e-2  # the input has none of it

"""LTM on slabs of the grid, CPU side: the slab restatement (tests/slab_ltm_numpy.py) adds up to the whole-grid
restatements, and the bindings of abz_rule_ltm_halo.  The device kernels are checked in test_gpu_ltm_slab.py."""
import os
import re

import numpy as np
import pytest

import abz_oracle as orc
import bloechl_numpy as bn
import ltm_numpy as ln
import slab_ltm_numpy as sn
import wltm_numpy as wn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    "int3-5x5": (lambda: orc.tb_integer(3), 5, 5),     # every slab is one plane, the last one's halo wraps to plane 0
    "int3-12x5": (lambda: orc.tb_integer(3), 12, 5),   # slabs of 2, 2, 3, 2, 3 planes
    "graphene-13x3": (orc.tb_graphene, 13, 3),
    "int2-7x7": (lambda: orc.tb_integer(2), 7, 7),
}


def energies(eig):
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    return np.concatenate([[lo - 0.1 * w, np.nextafter(lo, -np.inf), lo], np.linspace(lo, hi, 23) + 1e-3 / 7 * w, [hi, hi + 0.1 * w]])


def test_slab_partition_of_12_by_5():
    assert [b - a for a, b in sn.slabs(12, 5)] == [2, 2, 3, 2, 3]
    assert sum(a == b for a, b in sn.slabs(5, 7)) == 2  # more ranks than planes: empty slabs


@pytest.mark.parametrize("name", list(CASES))
def test_slabs_add_up_to_the_whole_grid(name):
    """The slab sums of the helper against ltm_numpy.ltm of the whole grid, 1e-14 max(1, max|ref|) (both are math.fsum
    of the same terms, in W pieces or in one; seen: at most 4.4e-16)."""
    make, npt, W = CASES[name]
    eig = ln.grid_eigenvalues(make(), npt)
    Es = energies(eig)
    g_ref, N_ref = ln.ltm(eig, Es)
    g, N = np.zeros(len(Es)), np.zeros(len(Es))
    below = Es < eig.min()
    assert below.sum() == 2
    sizes = []
    for z0, z1 in sn.slabs(npt, W):
        gs, Ns = sn.ltm(sn.extend(eig, z0, z1), Es)
        assert np.all(Ns[below] == 0.0) and np.all(gs[below] == 0.0)  # exactly 0 below the bands on every slab
        g += gs
        N += Ns
        sizes.append(z1 - z0)
    assert sum(sizes) == npt
    dg, dN = np.abs(g - g_ref).max(), np.abs(N - N_ref).max()
    print(f"slab sums {name} slabs {sizes}: g {dg:.2e} N {dN:.2e}")
    assert dg <= 1e-14 * max(1.0, np.abs(g_ref).max())
    assert dN <= 1e-14 * max(1.0, np.abs(N_ref).max())
    assert abs(N[-1] - eig.shape[-1]) <= 1e-12 * eig.shape[-1]


@pytest.mark.parametrize("name", list(CASES))
def test_energy_weighted_slabs_add_up(name):
    """g_A, N_A and the corrected N_A with A = e against wltm_numpy.wltm / bloechl_numpy.correction of the whole grid,
    1e-12 max(1, max|ref|)."""
    make, npt, W = CASES[name]
    eig = ln.grid_eigenvalues(make(), npt)
    Es = energies(eig)
    g_ref, N_ref = wn.wltm(eig, eig, Es)
    c_ref = bn.correction(eig, eig, Es)
    g, N, c = np.zeros_like(g_ref), np.zeros_like(N_ref), np.zeros_like(c_ref)
    below = Es < eig.min()
    for z0, z1 in sn.slabs(npt, W):
        ext = sn.extend(eig, z0, z1)
        sx = sn.sorted_simplices(ext, ext)
        gs, Ns = sn.wltm_from(sx, Es)
        cs = bn.correction_from(sx, Es)
        assert np.all(Ns[below] == 0.0) and np.all(cs[below] == 0.0)
        g += gs
        N += Ns
        c += cs
    for label, u, ref in (("g_A", g, g_ref), ("N_A", N, N_ref), ("corrected N_A", N + c, N_ref + c_ref)):
        dev = np.abs(u - ref).max()
        print(f"energy-weighted slab sums {name} {label}: {dev:.2e}")
        assert dev <= 1e-12 * max(1.0, np.abs(ref).max()), (name, label, dev)


def test_ltm_halo_bindings():
    import autobzcore.jl_amd as abz
    from autobzcore.jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "abzhip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "AutoBZCoreHIP.jl")).read()
    name = "abz_rule_ltm_halo"
    assert re.search(r"^int abz_rule_ltm_halo\(abz_rule\* r\);", hdr, flags=re.M)
    assert name in L.PROTOTYPES
    assert hasattr(L.lib(), name)
    assert ":" + name in jl
    defs = {k: int(v) for k, v in re.findall(r"^#define (ABZ_\w+) (-?\d+)\b", hdr, flags=re.M)}
    assert defs["ABZ_K_COUNT"] == 8 and defs["ABZ_VERSION"] == 502
    assert callable(getattr(abz.DeviceRule, "ltm_halo", None))
    assert "LTM" in abz.dist.kshard.__doc__

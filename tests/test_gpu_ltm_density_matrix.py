"""The density matrix rho_pq(E) = sum_k sum_b w_b(k; E) U_pb conj(U_qb) on the device (abz_rule_ltm_density_matrix;
ltm_dens_lane_kernel / ltm_dens_rows_kernel of kernels_ltm_dens.hip; DeviceRule.ltm_density_matrix, dos.density_matrix) against
the restatement tests/densmat_numpy.py, against the route it replaces (ltm_projectors in groups + ltm_node_weights_dot), and its
identities, repeatability, refusals and what it leaves alone.

Shapes: the smallest that reach every path --
    1 band    1-D, npt 2 and 65        N = 1, no H
    2, 3, 4   5^3 (3 bands also 17^2)  one node per lane, padded rows
    5         1-D grid of 40           NP = 8: two passes of 32 slots, the second ragged
    9         17^2                     NP = 16: a ragged second pass
    17        5^3                      NP = 32: 15 idle lanes per node
    32        3^3                      NP = 32: no idle lanes
    3 (SVO)   8^3                      a real Wannier series
Energies: test_gpu_ltm_node_weights.energy_list (below and above all bands, band edges, a node's eigenvalue, inside the bands
in no order, one twice) in calls of 1, 5 and 16, for the three kinds of weights.

Bounds.  Against the restatement fed the exported eigenvalues and LAPACK's projectors of the exported H (the generic series, which
have no degenerate levels; not SVO): 1e-10 max(1, max|ref|), the bound of the projector tests.  Fed the device's own exported
projectors (n <= 4, SVO among them): the parity bound 1e-9 max(1, max|ref|).  Against the route of projector groups and dots:
1e-12 max(1, max|ref|), summation order only.  tr rho and diag rho against the scans: two routes through the tetrahedron method,
the parity bound 1e-9 max(1, max|ref|).  Above the bands: 1e-13.  A multi-energy call against single-energy calls:
1e-13 max(1, max|rho|).  Degenerate levels: 1e-8 max(1, max|H|), as in the projector tests."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import abz_oracle as orc
import densmat_numpy as dm
import gloc_ltm_numpy as gl
import ltm_numpy as ln
import nodew_numpy as nw
from test_gpu_ltm import product_series
from test_gpu_ltm_green_matrix import all_pairs, bits, device_tensor, groups_of
from test_gpu_ltm_node_weights import CALLS, KIND_ARGS, energy_list, read_block
from test_gpu_parity import rand_series
from test_ltm_cpu import MODELS

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CASES = ["int1_2", "int1_65", "syn2_5", "syn3_5", "rand3_17", "syn4_5", "rand5_40", "rand9_17", "syn17_5", "syn32_3", "svo_8"]


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def make_series(abz, name):
    """(series, npt) of the table above"""
    kind, npt = name.split("_")
    npt = int(npt)
    if kind == "int1":
        return product_series(abz, MODELS["int1"][0]()), npt
    if kind == "svo":
        return abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz")), npt
    if kind.startswith("syn"):
        return product_series(abz, orc.synthetic_wannier(int(kind[3:]), rmax=2, seed=7)), npt
    n = int(kind[4:])
    dims = {3: (3, 3), 5: (5,), 9: (3, 5)}[n]
    c, first = rand_series(np.random.default_rng(100 * n + 5), dims, n, hermitian=True)
    return abz.FourierSeries(c, period=1.0, first=first, ndim=len(dims)), npt


_SHARED = {}


def shared(abz, name):
    """Per case, made once: the rule (H and eigenvalues), its exports, 16 energies, and the device's rho of the 16 for each kind"""
    if name not in _SHARED:
        s, npt = make_series(abz, name)
        rule = abz.DeviceRule(s.device(), npt, None, abz._lib.WANT_H | abz._lib.WANT_EIG)
        ex = rule.export(x=False, w=False, H=True, eig=True)
        eig = ln.rule_eigenvalues(rule)
        n = eig.shape[-1]
        H = ex["H"].reshape(eig.shape[:-1] + (n, n)) if n > 1 else np.ones(eig.shape[:-1] + (1, 1))
        Es = energy_list(eig, np.random.default_rng(5))
        rho = {kind: rule.ltm_density_matrix(Es, **kw) for kind, kw in KIND_ARGS.items()}
        _SHARED[name] = dict(s=s, npt=npt, rule=rule, eig=eig, H=H, Es=Es, rho=rho, n=n)
    return _SHARED[name]


def check(u, ref, rel, what):
    u, ref = np.asarray(u), np.asarray(ref)
    assert u.shape == ref.shape and u.dtype == np.complex128 and np.all(np.isfinite(bits(u))), (what, u.shape, ref.shape)
    dev, bound = float(np.abs(u - ref).max()), rel * max(1.0, float(np.abs(ref).max()))
    print(f"density matrix {what}: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)


def parent_route(rule):
    """rho [nE, n, n] of the resident weights by the route before this kernel: projectors in groups of at most 16 components,
    a dot per group, composed on the host"""
    n = rule.dev.s.n
    nE = rule.ltm_node_weights_ptr()[2]
    rho = np.zeros((nE, n, n), dtype=np.complex128)
    for group in groups_of(all_pairs(n)):
        rule.ltm_projectors(group)
        dot = rule.ltm_node_weights_dot()
        c = 0
        for p, q in group:
            if p == q:
                rho[:, p, p] = dot[:, c]
                c += 1
            else:
                rho[:, p, q] = dot[:, c] + 1j * dot[:, c + 1]
                rho[:, q, p] = dot[:, c] - 1j * dot[:, c + 1]
                c += 2
    rule.ltm_elements(None)
    return rho


# ---------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("name", [c for c in CASES if c != "svo_8"])
def test_density_matrix_matches_restatement_with_lapack_projectors(abz, name):
    """Generic series without degenerate levels.  (SVO's t2g bands are exactly degenerate on lines and planes of the grid: the
    weights of the degenerate bands differ there, so rho depends on the basis the solver picks inside the level, and LAPACK picks
    another one.  SVO is compared with the device's own projectors below.)"""
    sh = shared(abz, name)
    rule, eig, Es, n = sh["rule"], sh["eig"], sh["Es"], sh["n"]
    P = gl.projector_tensor(sh["H"])
    simp = nw.simplices(eig)
    for kind, kw in KIND_ARGS.items():
        ref = dm.contract(nw.node_weights_from(simp, eig.shape, Es, kind), P)
        check(sh["rho"][kind], ref, 1e-10, f"{name} {kind} nE=16 against LAPACK's projectors")
        for nE, pick in CALLS.items():
            if nE == 16:
                continue
            rho = rule.ltm_density_matrix(Es[pick], **kw)
            assert rho.shape == (nE, n, n)
            check(rho, ref[pick], 1e-10, f"{name} {kind} nE={nE} against LAPACK's projectors")


@pytest.mark.parametrize("name", ["int1_65", "syn2_5", "syn3_5", "rand3_17", "syn4_5", "svo_8"])
def test_density_matrix_matches_restatement_with_device_projectors(abz, name):
    sh = shared(abz, name)
    rule, eig, Es, n = sh["rule"], sh["eig"], sh["Es"], sh["n"]
    P = device_tensor(rule, all_pairs(n), n).reshape((n, n) + eig.shape)
    rule.ltm_elements(None)
    simp = nw.simplices(eig)
    for kind in KIND_ARGS:
        ref = dm.contract(nw.node_weights_from(simp, eig.shape, Es, kind), P)
        check(sh["rho"][kind], ref, 1e-9, f"{name} {kind} against the device's own projectors")


# ---------------------------------------------------------------- 2. against the route it replaces
@pytest.mark.parametrize("name", ["int1_65", "syn2_5", "syn3_5", "rand3_17", "syn4_5", "rand5_6", "rand5_40", "rand9_17", "syn17_5", "syn32_3", "svo_8"])
def test_density_matrix_matches_projector_groups_and_dots(abz, name):
    if name == "rand5_6":  # 5 + 20 components: two groups
        c, first = rand_series(np.random.default_rng(305), (3, 3), 5, hermitian=True)
        rule = abz.DeviceRule(abz.FourierSeries(c, period=1.0, first=first, ndim=2).device(), 6, None, abz._lib.WANT_EIG)
        Es = energy_list(ln.rule_eigenvalues(rule), np.random.default_rng(5))
        assert len(groups_of(all_pairs(5))) == 2
    else:
        sh = shared(abz, name)
        rule, Es = sh["rule"], sh["Es"]
    for kind, kw in KIND_ARGS.items():
        for nE, pick in CALLS.items():
            if nE == 5 and rule.dev.s.n > 16:
                continue  # (the groups of 17 and 32 bands: one and sixteen energies are enough)
            rho = rule.ltm_density_matrix(Es[pick], **kw)
            check(rho, parent_route(rule), 1e-12, f"{name} {kind} nE={nE} against projector groups + dot")
    if name == "rand5_6":
        rule.close()


# ---------------------------------------------------------------- 3. identities
@pytest.mark.parametrize("name", CASES)
def test_density_matrix_identities(abz, name):
    sh = shared(abz, name)
    rule, eig, Es, n = sh["rule"], sh["eig"], sh["Es"], sh["n"]
    lo, hi = float(eig.min()), float(eig.max())
    assert Es[0] < lo and Es[1] > hi
    eye = np.eye(n)
    for kind, kw in KIND_ARGS.items():
        rho = sh["rho"][kind]
        # Hermitian to the bit, a real diagonal
        assert np.array_equal(bits(rho), bits(np.conj(rho.transpose(0, 2, 1)))), (name, kind)
        assert np.all(np.diagonal(rho, axis1=1, axis2=2).imag == 0.0)
        # nothing below the bands; the identity above them (nothing, for the DOS weights)
        assert np.all(bits(rho[0]) == 0.0), (name, kind)
        top = float(np.abs(rho[1] - (eye if kind != "dos" else 0.0)).max())
        print(f"density matrix {name} {kind}: |rho - I| above the bands {top:.3e} (bound 1e-13)")
        assert top <= (1e-13 if kind != "dos" else 0.0), (name, kind, top)
        # the trace is the scan's N(E) or g(E) (the correction of A = 1 is zero)
        scan = rule.ltm(Es, states=kw["states"])
        check(np.trace(rho, axis1=1, axis2=2), scan.astype(np.complex128), 1e-9, f"{name} {kind} tr rho against abz_rule_ltm")
        # two calls: the same bits
        again = rule.ltm_density_matrix(Es, **kw)
        assert np.array_equal(bits(again), bits(rho)), (name, kind)
        assert np.array_equal(bits(rule.ltm_density_matrix()), bits(rho))  # ... and the resident weights once more
        # single-energy calls
        worst = 0.0
        for i in (2, 4, 8, 15):
            one = rule.ltm_density_matrix(Es[i:i + 1], **kw)
            worst = max(worst, float(np.abs(one[0] - rho[i]).max()) / max(1.0, float(np.abs(rho[i]).max())))
        print(f"density matrix {name} {kind}: 16 energies against single calls {worst:.3e} (bound 1e-13)")
        assert worst <= 1e-13, (name, kind, worst)
    # the diagonal is the scan with orbital weights (at most 16 of them per attach)
    for kind, kw in KIND_ARGS.items():
        diag = np.diagonal(sh["rho"][kind], axis1=1, axis2=2)
        for o0 in range(0, n, 16):
            orbs = list(range(o0, min(n, o0 + 16)))
            rule.ltm_orbitals(orbs)
            scan = rule.ltm(Es, elements="attached", **kw)
            check(diag[:, orbs], scan.astype(np.complex128), 1e-9, f"{name} {kind} diag rho against the scan of orbital weights {orbs[0]}..{orbs[-1]}")
    rule.ltm_elements(None)


# ---------------------------------------------------------------- 4. degenerate levels
def test_density_matrix_of_degenerate_levels(abz):
    """H = Q (I_2 x h(k)) Q^dagger, every level twice: rho = Q (I_2 x rho_h) Q^dagger.  Only sums over a level are defined."""
    L = abz._lib
    rng = np.random.default_rng(23)
    c3, first = rand_series(rng, (3, 3, 3), 3, hermitian=True)
    q, _ = np.linalg.qr(rng.standard_normal((6, 6)) + 1j * rng.standard_normal((6, 6)))
    c = np.einsum("ab,...bc,dc->...ad", q, np.kron(np.eye(2), c3), q.conj())
    c = 0.5 * (c + np.conj(np.swapaxes(c[::-1, ::-1, ::-1], -1, -2)))  # exactly Hermitian, degenerate to rounding
    r3 = abz.DeviceRule(abz.FourierSeries(c3, period=1.0, first=first).device(), 5, None, L.WANT_H | L.WANT_EIG)
    r6 = abz.DeviceRule(abz.FourierSeries(c, period=1.0, first=first).device(), 5, None, L.WANT_H | L.WANT_EIG)
    eig3 = ln.rule_eigenvalues(r3)
    H3 = r3.export(x=False, w=False, H=True)["H"].reshape(eig3.shape[:-1] + (3, 3))
    H6 = r6.export(x=False, w=False, H=True)["H"]
    lo, hi = float(eig3.min()), float(eig3.max())
    Es = np.concatenate([[lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo)], lo + (hi - lo) * rng.random(5)])
    bound = 1e-8 * max(1.0, float(np.abs(H6).max()))
    for kind, kw in KIND_ARGS.items():
        rho_h = dm.density_matrix(eig3, H3, Es, kind)
        ref = np.einsum("ab,ebc,dc->ead", q, np.stack([np.kron(np.eye(2), m) for m in rho_h]), q.conj())
        rho = r6.ltm_density_matrix(Es, **kw)
        dev = float(np.abs(rho - ref).max())
        print(f"density matrix, degenerate 3 x 2, {kind}: max dev {dev:.3e} (bound {bound:.1e})")
        assert dev <= bound, (kind, dev, bound)
    r3.close()
    r6.close()


# ---------------------------------------------------------------- 5. where H comes from
@pytest.mark.parametrize("name", ["syn3_5", "rand9_17"])
def test_density_matrix_does_not_depend_on_the_h_source(abz, name):
    L = abz._lib
    sh = shared(abz, name)
    for want in (L.WANT_EIG, L.WANT_H | L.WANT_EIG | L.WANT_H_COMPACT):
        rule = abz.DeviceRule(sh["s"].device(), sh["npt"], None, want)
        for kind, kw in KIND_ARGS.items():
            assert np.array_equal(bits(rule.ltm_density_matrix(sh["Es"], **kw)), bits(sh["rho"][kind])), (name, want, kind)
        rule.close()


# ---------------------------------------------------------------- 6. what a call leaves alone
@pytest.mark.parametrize("name,want", [("syn3_5", "eig"), ("rand9_17", "h")])
def test_density_matrix_leaves_elements_and_weights_alone(abz, name, want):
    L = abz._lib
    sh = shared(abz, name)
    rule = abz.DeviceRule(sh["s"].device(), sh["npt"], None, L.WANT_EIG if want == "eig" else L.WANT_H | L.WANT_EIG)
    A = np.random.default_rng(8).standard_normal((2, rule.nk, sh["n"]))
    rule.ltm_elements(A)
    rule.ltm_node_weights(sh["Es"][:5], export=False)
    ptr, block = rule.ltm_node_weights_ptr(), read_block(abz, rule)
    rho = rule.ltm_density_matrix()
    assert rho.shape == (5, sh["n"], sh["n"]) and np.array_equal(bits(rho), bits(sh["rho"]["states"][:5]))
    assert rule.ltm_node_weights_ptr() == ptr and np.array_equal(read_block(abz, rule), block)
    assert rule._ltm_ncomp == 2 and np.array_equal(rule.ltm_elements_export(), A)
    rule.close()


def test_density_matrix_beside_a_dos_cache(abz):
    h = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    bz = abz.load_bz(abz.FBZ(), 3.85856 * np.eye(3))
    Es = np.array([12.2, 12.6, 13.1])
    orb = abz.dos.init(abz.DOSProblem(h, Es, bz), abz.LTM(npt=8, elements="orbitals", eigenvectors="device"))
    u1 = abz.dos.solve_(orb).u
    owner = orb.cacheval._ltm_owner
    rho = orb.cacheval.ltm_density_matrix(Es)
    assert rho.shape == (3, 3, 3) and orb.cacheval._ltm_ncomp == 3 and orb.cacheval._ltm_owner is owner
    u2 = abz.dos.solve_(orb).u
    assert u2.shape == (3, 3) and np.array_equal(u1, u2)


# ---------------------------------------------------------------- 7. the front end
def test_dos_density_matrix(abz):
    h = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    bz = abz.load_bz(abz.FBZ(), 3.85856 * np.eye(3))
    cache = abz.dos.init(abz.DOSProblem(h, 0.0, bz), abz.LTM(npt=8))
    rule = cache.cacheval
    nstates, tol = 1.0, 1e-10
    E_F, N_F = abz.dos.fermi_level(cache, nstates)
    rho, E = abz.dos.density_matrix(cache, nstates=nstates)
    assert rho.shape == (3, 3) and rho.dtype == np.complex128 and E == E_F
    # fermi_level: N crosses nstates inside (E_F - tol, E_F], so N(E_F) - nstates <= g tol (+ its own 1e-12 slack); tr rho = N(E_F)
    g = rule.ltm(np.array([E_F]))[0]
    tr = float(np.trace(rho).real)
    print(f"dos.density_matrix: tr rho - nstates = {tr - nstates:.3e} (g tol = {g * tol:.1e}), tr rho - N_F = {tr - N_F:.3e}")
    assert abs(tr - nstates) <= g * tol + 1e-9 * max(1.0, nstates) and abs(tr - N_F) <= 1e-9
    assert np.array_equal(bits(rho), bits(np.conj(rho.T)))
    sub, _ = abz.dos.density_matrix(cache, nstates=nstates, orbitals=[2, 0])
    assert np.array_equal(bits(sub), bits(rho[[2, 0]][:, [2, 0]]))
    # a list of energies, the spectral-density matrix, a scalar energy, a problem instead of a cache
    Es = np.array([12.3, 12.9])
    rg, Eg = abz.dos.density_matrix(cache, E=Es, kind="dos")
    assert rg.shape == (2, 3, 3) and np.array_equal(Eg, Es)
    check(np.trace(rg, axis1=1, axis2=2), rule.ltm(Es).astype(np.complex128), 1e-9, "spectral-density matrix: trace against the DOS")
    r1, E1 = abz.dos.density_matrix(cache, E=float(E_F))
    assert E1 == E_F and np.array_equal(bits(r1), bits(rho))
    rc, _ = abz.dos.density_matrix(cache, nstates=nstates, correction=True)
    check(np.trace(rc[None], axis1=1, axis2=2), np.array([N_F], dtype=np.complex128), 1e-9, "corrected occupations: trace")
    assert np.abs(rc - rho).max() > 0.0
    rp, _ = abz.dos.density_matrix(abz.DOSProblem(h, 0.0, bz), E=Es[:1])
    assert rp.shape == (1, 3, 3)
    # mutate in place and set isfresh: H -> H / 2 gives the same rho at E / 2 (a power of two: every step scales exactly)
    h.c[...] = h.c * 0.5
    cache.isfresh = True
    r2, _ = abz.dos.density_matrix(cache, E=0.5 * E_F)
    assert not cache.isfresh
    check(r2, rho, 1e-12, "density_matrix follows the series")
    assert np.abs(abz.dos.density_matrix(cache, E=float(E_F))[0] - rho).max() > 1e-3


# ---------------------------------------------------------------- 8. refusals
def test_density_matrix_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s = product_series(abz, orc.synthetic_wannier(3, rmax=2, seed=7))
    dev = s.device()
    npt = 4
    Es = np.array([0.5, 1.5, -0.5])
    pE = Es.ctypes.data_as(L.c_f64p)
    out = np.full(2 * 33 * 33 * 3, -99.0)
    pout = out.ctypes.data_as(L.c_f64p)

    def refused(rc, code, words=None):
        msg = lib.abz_last_error()
        assert rc == code and len(msg) > 0, (rc, code, msg)
        assert words is None or words in msg, msg
        assert np.all(out == -99.0)  # nothing was written

    def keeps(rule, A, ptr, block, rc, code, words=None):
        refused(rc, code, words)
        assert np.array_equal(rule.ltm_elements_export(), A)
        assert rule.ltm_node_weights_ptr() == ptr and np.array_equal(read_block(abz, rule), block)

    # rules that are not a whole periodic grid, or hold no eigenvalues
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, npt, cub.syms, L.WANT_EIG)
    refused(lib.abz_rule_ltm_density_matrix(sym._h, pout), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    idx, w = abz.symptr_rule(npt, 3, cub.syms)
    irr, slab = C.c_void_p(), C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, npt, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(irr)))
    refused(lib.abz_rule_ltm_density_matrix(irr, pout), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    assert lib.abz_rule_destroy(irr) == 0
    L.check(lib.abz_ptr_rule_build_slab(dev.h, npt, 1, 3, L.WANT_EIG, C.byref(slab)))
    refused(lib.abz_rule_ltm_density_matrix(slab, pout), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    L.check(lib.abz_rule_ltm_halo(slab))
    refused(lib.abz_rule_ltm_density_matrix(slab, pout), L.ERR_UNSUPPORTED, b"slab")
    assert lib.abz_rule_destroy(slab) == 0
    honly = abz.DeviceRule(dev, npt, None, L.WANT_H)
    refused(lib.abz_rule_ltm_density_matrix(honly._h, pout), L.ERR_ARG, b"ABZ_WANT_EIG")
    honly.close()
    # an unfolded rule holds weights and elements, but no H(k)
    unf = sym.unfold()
    A = np.random.default_rng(1).standard_normal((2, unf.nk, 3))
    unf.ltm_elements(A)
    unf.ltm_node_weights(Es, export=False)
    keeps(unf, A, unf.ltm_node_weights_ptr(), read_block(abz, unf), lib.abz_rule_ltm_density_matrix(unf.h, pout), L.ERR_UNSUPPORTED, b"unfolded")
    unf.close()
    sym.close()
    # a rule that qualifies: no weights yet, a null out
    full = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    A = np.random.default_rng(2).standard_normal((2, full.nk, 3))
    full.ltm_elements(A)
    refused(lib.abz_rule_ltm_density_matrix(full.h, pout), L.ERR_ARG, b"holds no integration weights")
    with pytest.raises(ValueError, match="holds no weights"):
        full.ltm_density_matrix()
    full.ltm_node_weights(Es, export=False)
    ptr, block = full.ltm_node_weights_ptr(), read_block(abz, full)
    keeps(full, A, ptr, block, lib.abz_rule_ltm_density_matrix(full.h, None), L.ERR_ARG, b"null out")
    refused(lib.abz_rule_ltm_density_matrix(None, pout), L.ERR_ARG, b"null rule handle")
    with pytest.raises(ValueError, match="twice"):
        full.ltm_density_matrix(orbitals=[1, 1])
    with pytest.raises(ValueError, match="outside"):
        full.ltm_density_matrix(orbitals=[0, 3])
    with pytest.raises(ValueError):
        full.ltm_density_matrix(orbitals=[])
    # a valid call afterwards
    assert lib.abz_rule_ltm_density_matrix(full.h, pout) == 0
    got = out[:2 * 9 * 3].view(np.complex128).reshape(3, 3, 3)
    assert np.all(out[2 * 9 * 3:] == -99.0) and np.array_equal(bits(got), bits(full.ltm_density_matrix()))
    assert np.array_equal(full.ltm_elements_export(), A) and full.ltm_node_weights_ptr() == ptr
    out[:] = -99.0
    full.close()
    # above 32 bands there is no kernel
    sn = product_series(abz, orc.synthetic_wannier(33, rmax=2, seed=7))
    rule = abz.DeviceRule(sn.device(), 3, None, L.WANT_EIG)
    A = np.ones((1, rule.nk, 33))
    rule.ltm_elements(A)
    rule.ltm_node_weights(Es, export=False)
    keeps(rule, A, rule.ltm_node_weights_ptr(), read_block(abz, rule), lib.abz_rule_ltm_density_matrix(rule.h, pout), L.ERR_UNSUPPORTED, b"33 bands")
    rule.close()
    # a series that is not Hermitian
    c, first = rand_series(np.random.default_rng(9), (3, 3, 3), 3, hermitian=False)
    rule = abz.DeviceRule(abz.FourierSeries(c, period=1.0, first=first).device(), npt, None, L.WANT_H | L.WANT_EIG)
    A = np.ones((1, rule.nk, 3))
    rule.ltm_elements(A)
    rule.ltm_node_weights(Es, export=False)
    keeps(rule, A, rule.ltm_node_weights_ptr(), read_block(abz, rule), lib.abz_rule_ltm_density_matrix(rule.h, pout), L.ERR_ARG, b"Hermitian")
    rule.close()


def test_density_matrix_python_refusals(abz):
    L = abz._lib
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.dos.init(abz.DOSProblem(s, 0.0, cub), abz.LTM(npt=8, symmetric=True))
    with pytest.raises(ValueError, match="symmetric"):
        abz.dos.density_matrix(sym, E=0.5)
    with pytest.raises(ValueError, match="LTM cache"):
        abz.dos.density_matrix(abz.dos.init(abz.DOSProblem(s, 0.0, cub), abz.GGR(npt=8)), E=0.5)
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        rule = dev.rule(8, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError, match="halo"):
            rule.ltm_density_matrix([0.5])
        rule.ltm_halo()
        with pytest.raises(NotImplementedError, match="ltm_density_matrix"):
            rule.ltm_density_matrix([0.5])
        with pytest.raises(NotImplementedError, match="density_matrix on a k-sharded"):
            abz.dos.density_matrix(abz.DOSProblem(s, 0.0, bz), E=0.5)
    finally:
        dev.kshard, dev.allreduce = None, None


def test_density_matrix_is_accounted(abz):
    """abz_mem_info: a call, its transient H-only rule and a refusal leave nothing behind, and the bytes and blocks return to
    their value when the rule goes."""
    L = abz._lib
    s, npt = make_series(abz, "rand9_17")
    dev = s.device()
    info = lambda: (dev.ctx.mem_info()[0], dev.ctx.mem_info()[4])
    Es = np.array([0.1, -0.4, 0.7])
    out = np.zeros((3, 9, 9), dtype=np.complex128)

    def cycle():
        m0 = info()
        rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
        rule.ltm_node_weights(Es, export=False)
        m1 = info()
        assert L.lib().abz_rule_ltm_density_matrix(rule.h, None) == L.ERR_ARG
        assert info() == m1
        rule.ltm_density_matrix()  # with a transient rule for H(k)
        m2 = info()
        rule.ltm_density_matrix()
        m3 = info()
        rule.close()
        return m0, m1, m2, m3, info()

    gc.collect()
    gc.disable()
    try:
        cycle()  # the context's and the series' scratch buffers grow once
        m0, m1, m2, m3, m4 = cycle()
    finally:
        gc.enable()
    print(f"mem (bytes, blocks): before {m0}, rule with weights {m1}, after a call {m2}, after another {m3}, destroyed {m4}")
    assert m2 == m1 and m3 == m1 and m4 == m0


# ---------------------------------------------------------------- profiling
@pytest.mark.parametrize("name", ["syn3_5", "rand9_17"])
def test_density_matrix_launches_are_profiled(abz, name):
    """One ProfScope of ABZ_K_EIG per call around the contraction kernels (four launches for 16 energies of 3 bands, one for 9)."""
    L = abz._lib
    sh = shared(abz, name)
    ctx = sh["rule"].dev.ctx
    sh["rule"].ltm_node_weights(sh["Es"], export=False)
    ctx.prof_enable(True, kernels=[L.K_EIG])
    try:
        ctx.prof_reset()
        sh["rule"].ltm_density_matrix()
        ms, launches = ctx.prof_read(L.K_EIG)
        assert launches == 1 and ms > 0.0
    finally:
        ctx.prof_enable(False)

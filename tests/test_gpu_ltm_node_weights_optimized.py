"""Integration weights of the optimized tetrahedron method on the device (abz_rule_ltm_node_weights_optimized;
ltm_opt_cornerw_kernel of kernels_ltm_opt_nodew.hip, ltm_opt_nodew_gather_kernel of ltm_opt_nodew_device.h) against the scatter-form restatement of
tests/optnodew_numpy.py, against the shipped scans of abz_rule_ltm_optimized, and their exact values, repeatability, slabs,
consumers (dot, fold, density matrix), lifetime and refusals.

Parity bound: the restatement is fed the rule's own exported eigenvalues, so only summation order, FMA contraction and the form
of the product (the kernel adds sum_j P_mj (x_j - x_m) to x_m) remain; the cases are those of
test_ltm_node_weights_optimized_cpu.py, whose f64 and longdouble evaluations agree to 1e-10 in nk w.  The bound is the project's
LTM parity bound applied to the O(1) quantity nk w,   |nk u - nk ref| <= 1e-9 max(1, max|nk ref|)   (check_nk of
test_gpu_ltm_node_weights.py).

Shapes: npt = 1, 2, 3 (the stencil on itself, one slab of wrapped planes), 5, 7, 8 (less than a block, odd, even), 17 with 3 bands
(row padded to 32, a ragged last block, 17 slabs under a cap of 1 MB)."""
import ctypes as C
import gc

import numpy as np
import pytest

import abz_oracle as orc
import densmat_numpy as dm
import gloc_ltm_numpy as gl
import ltm_numpy as ln
import nodew_numpy as nw
import optnodew_numpy as onw
import unfold_numpy as un
from test_gpu_ltm import product_series
from test_gpu_ltm_green_matrix import all_pairs, bits, device_tensor
from test_gpu_ltm_node_weights import check, check_nk, flat_band_series, on_nodes, read_block, series_of
from test_ltm_node_weights_optimized_cpu import CALLS, DEVICE_GRIDS, energy_list
from test_ltm_optimized_cpu import case_coefficients, case_elements
from test_ltm_unfold_cpu import model_sym_sets

pytestmark = pytest.mark.gpu

KINDS = {"dos": False, "states": True}
SWITCH = "ABZ_LTM_OPTW_CHUNK_MB"


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def case_rule(abz, n, npt, want=None):
    c, first = case_coefficients(n)
    s = abz.FourierSeries(c, period=1.0, first=first, ndim=3)
    return s, s.device().rule(npt, None, abz._lib.WANT_EIG if want is None else want)


# ---------------------------------------------------------------- 1. parity with the restatement
@pytest.mark.parametrize("n,npt", [(n, npt) for n in sorted(DEVICE_GRIDS) for npt in DEVICE_GRIDS[n]])
def test_optimized_node_weights_match_restatement(abz, n, npt):
    s, rule = case_rule(abz, n, npt)
    eig = ln.rule_eigenvalues(rule)
    Es = energy_list(eig)
    worst = 0.0
    for kind, states in KINDS.items():
        ref = on_nodes(rule, onw.node_weights(eig, Es, states))  # once per kind, for the calls of 1, 5 and 16
        for nE, pick in CALLS.items():
            W = rule.ltm_node_weights_optimized(Es[pick], states=states)
            assert W.shape == (nE, rule.nk, n)
            worst = max(worst, check_nk(W, ref[pick], rule.nk, f"optimized n={n} npt={npt} {kind} nE={nE}"))
            assert rule.ltm_node_weights_ptr()[2] == nE
    print(f"optimized nodew parity n={n} npt={npt}: worst deviation / bound = {worst:.3e}")


# ---------------------------------------------------------------- 2. exact values
@pytest.mark.parametrize("n,npt", [(1, 2), (3, 3), (3, 8), (3, 17)])
def test_optimized_node_weights_exact_values(abz, n, npt):
    s, rule = case_rule(abz, n, npt)
    eig = ln.rule_eigenvalues(rule)
    nk = rule.nk
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    # e' leaves the range of the eigenvalues by less than (1836 / 1260 - 1) / 2 = 0.23 of its width
    Es = np.array([lo - 0.3 * w, hi + 0.3 * w, lo + 0.4 * w])
    S = rule.ltm_node_weights_optimized(Es, states=True)
    G = rule.ltm_node_weights_optimized(Es, states=False)
    assert np.all(S[0] == 0.0) and not np.any(np.signbit(S[0]))  # below every e'
    assert np.all(G[0] == 0.0) and np.all(G[1] == 0.0)            # the DOS outside the bands
    dev = float(np.abs(nk * S[1] - 1.0).max())
    print(f"n={n} npt={npt}: max |nk w - 1| above every e' = {dev:.2e}")
    assert dev <= 1e-12
    assert np.abs(S[2]).max() > 0.0


def test_optimized_node_weights_of_an_exactly_flat_band(abz):
    """One band, e(k) = 0.25 to the bit (the model of test_green_optimized_flat_band): e' = x_m + sum P (x_j - x_m) keeps the
    value to the bit, every simplex is flat.  DOS weights: 0.0 at every energy, E = v included; STATES: 0.0 below v, and at
    E = v every simplex lies wholly below E, 6 x 20 x (rows of P summing to one) x 1/4 / (6 nk) = 1 / nk."""
    c = np.zeros((3, 3, 3, 1, 1), dtype=np.complex128)
    c[1, 1, 1, 0, 0] = 0.25
    s = abz.FourierSeries(c, period=1.0, first=(-1, -1, -1), ndim=3)
    rule = s.device().rule(6, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    v = float(eig.reshape(-1)[0])
    assert np.all(eig == v)
    Es = np.array([np.nextafter(v, -1.0), v, np.nextafter(v, 1.0), v - 1.0, v + 1.0])
    G = rule.ltm_node_weights_optimized(Es, states=False)
    S = rule.ltm_node_weights_optimized(Es, states=True)
    assert np.all(G == 0.0)
    assert np.all(S[0] == 0.0) and np.all(S[3] == 0.0)
    dev = float(np.abs(rule.nk * S[[1, 2, 4]] - 1.0).max())
    print(f"exactly flat band: max |nk w - 1| at E = v and above: {dev:.2e}")
    assert dev <= 1e-12


def test_optimized_node_weights_of_the_flat_band_model(abz):
    """diag(e, e, 0.25): the bands are stored ascending, so the flat level is band 0 where e > 0.25 and band 2 where e < 0.25, and
    the 3 x 3 eigen-solve returns it as q +- p x: 0.25 to a few ulp, not to the bit.  A weight comes from the simplices of the
    cells k - [-1, 2]^3, whose stencils reach k + [-3, 3]^3.  Where the band is flat on that whole neighbourhood every e' is
    0.25 to rounding, so away from that rounding -- at 0.25 -+ 1e-9 -- the DOS weight is 0.0, the STATES weight 0.0 below and
    1 / nk above.  E = 0.25 itself lies INSIDE the rounding of such a band (a window 1e-16 wide, a DOS weight of 1e16 or none):
    the exactly flat band above takes that energy."""
    npt = 14
    rule = flat_band_series(abz).device().rule(npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    nk = rule.nk
    whole = np.abs(eig - 0.25) <= 1e-14
    for ax in range(3):
        whole = np.logical_and.reduce([np.roll(whole, o, axis=ax) for o in range(-3, 4)])
    mask = whole.reshape(nk, 3)
    print(f"flat band model: {int(mask.sum())} entries with a flat neighbourhood; largest |e - 0.25| among them {np.abs(eig[whole] - 0.25).max():.1e}")
    assert mask.any()
    # What moved E = 0.25 itself to the exactly flat band above: the solver's flat level is not 0.25 to the bit.  Where a solver
    # does return it to the bit, E = 0.25 is asserted here as well.
    level = eig[np.abs(eig - 0.25) <= 1e-14]
    if np.abs(level - 0.25).max() == 0.0:
        G0 = rule.ltm_node_weights_optimized(np.array([0.25]), states=False)
        S0 = rule.ltm_node_weights_optimized(np.array([0.25]), states=True)
        assert np.all(G0[0][mask] == 0.0) and np.abs(nk * S0[0][mask] - 1.0).max() <= 1e-12
    Es = np.array([0.25 - 1e-9, 0.25 + 1e-9, -1.0, 2.0])
    G = rule.ltm_node_weights_optimized(Es, states=False)
    S = rule.ltm_node_weights_optimized(Es, states=True)
    assert np.all(G[:, mask] == 0.0)
    assert np.all(S[0][mask] == 0.0)
    dev = float(np.abs(nk * S[1][mask] - 1.0).max())
    print(f"flat band model: max |nk w - 1| at E = 0.25 + 1e-9: {dev:.2e}")
    assert dev <= 1e-12
    # the whole model against the restatement, away from 0.25
    away = np.array([-1.0, 2.0, 0.2, 0.3])
    for kind, states in KINDS.items():
        W = rule.ltm_node_weights_optimized(away, states=states)
        check_nk(W, on_nodes(rule, onw.node_weights(eig, away, states)), nk, f"flat band model {kind}")


# ---------------------------------------------------------------- 3. against the shipped scans
@pytest.mark.parametrize("name,npt", [("svo", 6), ("syn6", 5)])
def test_optimized_node_weights_against_the_shipped_scans(abz, name, npt):
    s = series_of(abz, name)
    rule = s.device().rule(npt, None, abz._lib.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    n = eig.shape[-1]
    Es = energy_list(eig)
    A = np.random.default_rng(2).standard_normal((16, rule.nk, n))
    rule.ltm_elements(A)
    eflat = eig.reshape(rule.nk, n)
    for kind, states in KINDS.items():
        scan = rule.ltm_optimized(Es, states=states, elements="attached")  # [16, 16]
        total = rule.ltm_optimized(Es, states=states)
        energy = rule.ltm_optimized(Es, states=states, elements="energy")[:, 0]
        for nE, pick in CALLS.items():
            W = rule.ltm_node_weights_optimized(Es[pick], states=states)
            dot = rule.ltm_node_weights_dot()
            assert dot.shape == (nE, 16)
            check(dot, scan[pick], f"{name} {kind} nE={nE} dot against ltm_optimized with elements")
            check(np.einsum("ekb,ckb->ec", W, A), scan[pick], f"{name} {kind} nE={nE} einsum(W, A) against ltm_optimized")
            check(W.sum(axis=(1, 2)), total[pick], f"{name} {kind} nE={nE} sum of the weights")
            check(np.einsum("ekb,kb->e", W, eflat), energy[pick], f"{name} {kind} nE={nE} sum w e")
    rule.ltm_elements(None)
    assert rule.ltm_node_weights_ptr()[2] == 16  # dropping ELEMENTS leaves the weights alone


# ---------------------------------------------------------------- 4. repeatability, padding, the block
@pytest.mark.parametrize("n,npt", [(3, 5), (3, 17)])
def test_optimized_node_weights_repeatable_and_padding_is_zero(abz, n, npt):
    s, rule = case_rule(abz, n, npt)
    eig = ln.rule_eigenvalues(rule)
    Es = energy_list(eig)
    rule.ltm_elements(case_elements(n, npt))
    for states in KINDS.values():
        for pick in CALLS.values():
            a = rule.ltm_node_weights_optimized(Es[pick], states=states)
            da = rule.ltm_node_weights_dot()
            block_a = read_block(abz, rule)
            b = rule.ltm_node_weights_optimized(Es[pick], states=states)
            db = rule.ltm_node_weights_dot()
            block = read_block(abz, rule)
            assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(da), bits(db)) and np.array_equal(bits(block_a), bits(block))
            assert np.all(block[:, :, npt:] == 0.0) and not np.any(np.signbit(block[:, :, npt:]))  # the padding columns: +0.0
            # the block is the export: plane i n + b of line l, column c = w_b(k = l npt + c; E_i)
            got = block[:, :, :npt].reshape(npt ** 2, len(pick), n, npt).transpose(1, 0, 3, 2).reshape(len(pick), rule.nk, n)
            assert np.array_equal(bits(got), bits(b))
            if len(pick) % 4 == 1:  # the last energy ran alone (NE = 1): the bits it has in a call of its own
                one = rule.ltm_node_weights_optimized(Es[pick[-1:]], states=states)
                assert np.array_equal(bits(one[0]), bits(b[-1]))
    assert rule.ltm_node_weights_optimized(Es[:5], export=False) is None and rule.ltm_node_weights_ptr()[2] == 5
    rule.ltm_elements(None)


# ---------------------------------------------------------------- 5. slabs: the same bits for every cap
def test_optimized_node_weights_do_not_depend_on_the_chunk(abz, monkeypatch):
    """npt = 17, 3 bands: a plane of cells takes 24 x 3 x 8 x 289 B = 166 KB per energy.  Cap 1 MB: groups of 4 energies in 17
    slabs of one plane, single energies in slabs of 3; 4 MB: groups of 4 in slabs of 3, single energies in one slab; no cap: one
    slab.  npt = 8 under 1 MB: groups of 4 in two slabs of 4 planes."""
    for npt, caps in ((17, ("1", "4", None)), (8, ("1", None))):
        s, rule = case_rule(abz, 3, npt)
        Es = energy_list(ln.rule_eigenvalues(rule))
        got = {}
        for cap in caps:
            if cap is None:
                monkeypatch.delenv(SWITCH, raising=False)
            else:
                monkeypatch.setenv(SWITCH, cap)
            got[cap] = [rule.ltm_node_weights_optimized(Es[pick], states=states) for states in KINDS.values() for pick in CALLS.values()]
        monkeypatch.delenv(SWITCH, raising=False)
        for cap in caps[:-1]:
            for a, b in zip(got[cap], got[None]):
                assert np.array_equal(bits(a), bits(b)), (npt, cap)


def test_chunk_switch_bounds_the_scratch(abz, monkeypatch):
    """The switch is read: on a fresh context under a cap of 1 MB the context's scratch (abz_mem_info) holds the S + 3 = 4 planes of a
    group of 4 energies, 8 x 24 x 3 x 4 x 4 x 17^2 B = 2.7 MB, and stays below the 17 planes of the whole grid, 11.3 MB, which the
    same call without a cap then reserves."""
    L = abz._lib
    lib = L.lib()
    npt, n = 17, 3
    c, _ = case_coefficients(n)
    c = np.ascontiguousarray(c)
    dims, first, per = np.array([3, 3, 3], dtype=np.int32), np.array([-1, -1, -1], dtype=np.int32), np.ones(3)
    Es = np.array([0.1, -0.3, 0.2, 0.0, 0.5])
    pE = Es.ctypes.data_as(L.c_f64p)
    plane = 8 * 24 * n * 4 * npt ** 2  # of a group of 4 energies
    ctx, s, full = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.check(lib.abz_ctx_create(0, C.byref(ctx)))
    L.check(lib.abz_series_create(ctx, c.view(np.float64).ctypes.data_as(L.c_f64p), 3, dims.ctypes.data_as(L.c_i32p),
                                  first.ctypes.data_as(L.c_i32p), per.ctypes.data_as(L.c_f64p), n, C.byref(s)))
    L.check(lib.abz_ptr_rule_build(s, npt, 0, None, None, L.WANT_EIG, C.byref(full)))
    try:
        monkeypatch.setenv(SWITCH, "1")
        L.check(lib.abz_rule_ltm_node_weights_optimized(full, pE, 5, L.LTM_STATES, None))
        capped = books(L, ctx)[2]
        monkeypatch.delenv(SWITCH, raising=False)
        L.check(lib.abz_rule_ltm_node_weights_optimized(full, pE, 5, L.LTM_STATES, None))
        whole = books(L, ctx)[2]
        print(f"scratch of the context: {capped} B under a cap of 1 MB (4 planes: {4 * plane} B), {whole} B without (17 planes: {npt * plane} B)")
        assert 4 * plane <= capped < npt * plane <= whole
    finally:
        monkeypatch.delenv(SWITCH, raising=False)
        assert lib.abz_rule_destroy(full) == 0 and lib.abz_series_destroy(s) == 0 and lib.abz_ctx_destroy(ctx) == 0


# ---------------------------------------------------------------- 6. unfolded rules and the fold
@pytest.mark.parametrize("name,npt", [("int3", 4), ("int3", 6), ("svo", 4), ("svo", 6)])
def test_optimized_node_weights_of_an_unfolded_rule_and_their_fold(abz, name, npt):
    L = abz._lib
    s = series_of(abz, name)
    dev = s.device()
    syms = model_sym_sets(abz, name, 3)["cubic"]
    src = abz.DeviceRule(dev, npt, syms, L.WANT_EIG)
    unf = src.unfold()
    full = dev.rule(npt, None, L.WANT_EIG)
    eig = ln.rule_eigenvalues(unf)
    n, nk, nirr = eig.shape[-1], unf.nk, src.nk
    lo, hi = float(eig.min()), float(eig.max())
    Es = np.concatenate([[lo - 0.4 * (hi - lo) - 0.1, hi + 0.4 * (hi - lo) + 0.1], lo + (hi - lo) * np.random.default_rng(6).random(5)])
    se = src.export(eig=True)
    node_of = un.orbit_map(npt, 3, syms, se["x"])  # the orbits on the host, from the exported nodes and the matrices
    for kind, states in KINDS.items():
        W = unf.ltm_node_weights_optimized(Es, states=states)
        check_nk(W, full.ltm_node_weights_optimized(Es, states=states), nk, f"{name} npt={npt} {kind} unfolded against the full build")
        ref = on_nodes(unf, onw.node_weights(eig, Es, states))
        check_nk(W, ref, nk, f"{name} npt={npt} {kind} unfolded against the restatement")
        fold = unf.ltm_node_weights_fold()
        assert fold.shape == (len(Es), nirr, n)
        fold_ref = np.zeros_like(fold)
        np.add.at(fold_ref, (slice(None), node_of), ref)
        # an orbit holds at most 48 points: the bound on nk w, for sums of up to 48 of them
        check_nk(fold, fold_ref, nk, f"{name} npt={npt} {kind} fold against the restatement's orbit sums")
        check(fold.sum(axis=(1, 2)), W.sum(axis=(1, 2)), f"{name} npt={npt} {kind} fold.sum against W.sum")
        assert np.array_equal(bits(fold), bits(unf.ltm_node_weights_fold()))


# ---------------------------------------------------------------- 7. the density matrix
@pytest.mark.parametrize("name,npt", [("svo", 6), ("syn6", 5)])
def test_density_matrix_of_optimized_weights(abz, name, npt):
    """rho = sum_k sum_b w U U^dagger with the optimized weights.  The reference with numpy's eigenvectors of the exported H(k) is
    densmat_numpy.contract of the restatement's weights and gloc_ltm_numpy.projector_tensor.  SVO's t2g bands are exactly
    degenerate on lines and planes of the grid, where the weights of the degenerate bands differ: rho then depends on the basis
    the solver picks inside the level (test_gpu_ltm_density_matrix.py), so SVO is also set against the device's own projectors."""
    L = abz._lib
    s = series_of(abz, name)
    rule = abz.DeviceRule(s.device(), npt, None, L.WANT_H | L.WANT_EIG)
    ex = rule.export(x=False, w=False, H=True, eig=True)
    eig = ln.rule_eigenvalues(rule)
    n = eig.shape[-1]
    H = ex["H"].reshape(eig.shape[:-1] + (n, n))
    Es = energy_list(eig)
    P_lapack = gl.projector_tensor(H)
    P_device = device_tensor(rule, all_pairs(n), n).reshape((n, n) + eig.shape)
    rule.ltm_elements(None)
    for kind, states in KINDS.items():
        rho = rule.ltm_density_matrix(Es, states=states, optimized=True)
        assert rho.shape == (16, n, n) and rho.dtype == np.complex128
        assert np.array_equal(bits(rho), bits(np.conj(rho.transpose(0, 2, 1))))  # Hermitian to the bit
        assert np.all(np.diagonal(rho, axis1=1, axis2=2).imag == 0.0)
        assert np.array_equal(bits(rho), bits(rule.ltm_density_matrix()))  # the resident weights once more
        check(np.trace(rho, axis1=1, axis2=2).real, rule.ltm_optimized(Es, states=states), f"{name} {kind} tr rho against ltm_optimized")
        Wref = onw.node_weights(eig, Es, states)
        dev = float(np.abs(rho - dm.contract(Wref, P_device)).max())
        bound = 1e-9 * max(1.0, float(np.abs(rho).max()))
        print(f"{name} {kind}: rho against the restatement with the device's projectors {dev:.3e} (bound {bound:.1e})")
        assert dev <= bound
        dev = float(np.abs(rho - dm.contract(Wref, P_lapack)).max())
        print(f"{name} {kind}: rho against the restatement with numpy's eigenvectors {dev:.3e} (bound {bound:.1e})")
        if name != "svo":
            assert dev <= bound
    # the diagonal is the optimized scan of the orbital weights
    for kind, states in KINDS.items():
        rho = rule.ltm_density_matrix(Es, states=states, optimized=True)
        rule.ltm_orbitals(list(range(n)))
        scan = rule.ltm_optimized(Es, states=states, elements="attached")
        check(np.diagonal(rho, axis1=1, axis2=2).real, scan, f"{name} {kind} diag rho against ltm_optimized of the orbital weights")
        rule.ltm_elements(None)
    with pytest.raises(ValueError, match="correction"):
        rule.ltm_density_matrix(Es, correction=True, optimized=True)
    rule.close()


# ---------------------------------------------------------------- 8. the front end
def test_optimized_integration_weights_front_end(abz):
    c, first = case_coefficients(3)
    s = abz.FourierSeries(c, period=1.0, first=first, ndim=3)
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    nstates, tol = 1.3, 1e-10
    cache = abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=8, optimized=True))
    rule = cache.cacheval
    E_F, N_F = abz.dos.fermi_level(cache, nstates)  # the optimized level: the cache's algorithm
    assert (E_F, N_F) == abz.dos.fermi_level(cache, nstates, optimized=True)
    W, E = abz.dos.integration_weights(cache, nstates=nstates, optimized=True)
    assert W.shape == (rule.nk, 3) and E == E_F
    g = rule.ltm_optimized(np.array([E_F]))[0]
    print(f"optimized occupations: sum W - nstates = {W.sum() - nstates:.3e} (g tol = {g * tol:.1e}), min nk w = {rule.nk * W.min():.3e}")
    assert abs(W.sum() - nstates) <= g * tol + 1e-9
    # the default is the linear rule whatever the cache's algorithm is: today's weights, bit for bit
    Wl, El = abz.dos.integration_weights(cache, nstates=nstates)
    assert El == E_F and np.array_equal(bits(Wl), bits(rule.ltm_node_weights(np.array([E_F]))[0]))
    assert np.array_equal(bits(abz.dos.integration_weights(cache, nstates=nstates, optimized=False)[0]), bits(Wl))
    assert abs(Wl.sum() - nstates) > 1e-6  # (which is why the keyword exists)
    # a list of energies, the DOS weights, a problem instead of a cache (LTM(): the linear level would be taken, none is here)
    Es = np.array([E_F - 0.2, E_F + 0.1])
    Wg, Eg = abz.dos.integration_weights(abz.DOSProblem(s, 0.0, bz), E=Es, kind="dos", optimized=True)
    assert Wg.shape == (2, 50 ** 3, 3) and np.array_equal(Eg, Es)
    check(Wg.sum(axis=(1, 2)), abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(optimized=True)).u, "DOS weights sum to the DOS of LTM(optimized=True)")
    # the density matrix: tr rho = nstates on the optimized rule
    ch = abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=8))
    rho, Er = abz.dos.density_matrix(ch, nstates=nstates, optimized=True)
    assert Er == E_F and abs(np.trace(rho).real - nstates) <= g * tol + 1e-9
    rho_l, El2 = abz.dos.density_matrix(ch, nstates=nstates)
    assert El2 == abz.dos.fermi_level(ch, nstates)[0] and El2 != E_F
    # fold=True works as today
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    s3 = product_series(abz, orc.tb_integer(3))
    csym = abz.dos.init(abz.DOSProblem(s3, 0.0, cub), abz.LTM(npt=8, symmetric=True))
    Wf, Ef = abz.dos.integration_weights(csym, nstates=0.4, fold=True, optimized=True)
    src = csym.cacheval.source
    assert Wf.shape == (src.nk, 1) and Ef == abz.dos.fermi_level(csym, 0.4, optimized=True)[0]
    gs = csym.cacheval.ltm_optimized(np.array([Ef]))[0]
    assert abs(Wf.sum() - 0.4) <= gs * tol + 1e-9
    with pytest.raises(ValueError, match="fold"):
        abz.dos.integration_weights(cache, E=0.1, fold=True, optimized=True)
    # a k-sharded series is refused before anything is built
    dev = s.device()
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        for f in (abz.dos.integration_weights, abz.dos.density_matrix):
            with pytest.raises(NotImplementedError, match="k-sharded"):
                f(abz.DOSProblem(s, 0.0, bz), E=0.1, optimized=True)
        r = dev.rule(8, None, abz._lib.WANT_EIG)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_node_weights_optimized(Es)
    finally:
        dev.kshard, dev.allreduce = None, None


# ---------------------------------------------------------------- 9. refusals
def test_optimized_node_weight_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s, full = case_rule(abz, 3, 4)
    dev = s.device()
    npt = 4
    Es = np.array([0.5, 1.5, -0.5])
    pE = Es.ctypes.data_as(L.c_f64p)
    out = np.full(16 * 3 * npt ** 3, -99.0)
    pout = out.ctypes.data_as(L.c_f64p)
    h = full._h
    kept = full.ltm_node_weights(Es)  # a previously resident block (the linear rule's)
    kept_ptr = full.ltm_node_weights_ptr()
    kept_block = read_block(abz, full)
    f = lib.abz_rule_ltm_node_weights_optimized

    def refused(rc, code, match=None):
        msg = lib.abz_last_error().decode()
        assert rc == code and len(msg) > 0, (rc, code, msg)
        assert match is None or match in msg, msg
        assert np.all(out == -99.0)  # nothing was written
        assert full.ltm_node_weights_ptr() == kept_ptr and np.array_equal(read_block(abz, full), kept_block)

    bad = np.array([0.5, np.nan, np.inf])
    refused(f(h, pE, 0, L.LTM_STATES, pout), L.ERR_ARG, "outside 1..16")
    refused(f(h, pE, 17, L.LTM_STATES, pout), L.ERR_ARG, "outside 1..16")
    refused(f(h, bad.ctypes.data_as(L.c_f64p), 2, L.LTM_STATES, pout), L.ERR_ARG, "not finite")
    refused(f(h, bad[[0, 2]].copy().ctypes.data_as(L.c_f64p), 2, L.LTM_DOS, pout), L.ERR_ARG, "not finite")
    refused(f(h, None, 3, L.LTM_STATES, pout), L.ERR_ARG)
    refused(f(h, pE, 3, L.LTM_STATES_CORRECTED, pout), L.ERR_ARG, "replaces the curvature correction")
    for what in (3, -1, 7):
        refused(f(h, pE, 3, what, pout), L.ERR_ARG, "what")
    # d = 2
    s2 = product_series(abz, orc.tb_integer(2))
    flat = abz.DeviceRule(s2.device(), 8, None, L.WANT_EIG)
    refused(f(flat._h, pE, 3, L.LTM_STATES, pout), L.ERR_UNSUPPORTED, "d = 2")
    with pytest.raises(NotImplementedError, match="d = 3"):
        flat.ltm_node_weights_optimized(Es)
    # a slab without and with its halo plane, irreducible nodes, a rule without eigenvalues
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    idx, w = abz.symptr_rule(npt, 3, cub.syms)
    irr, slab, halo = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, npt, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(irr)))
    L.check(lib.abz_ptr_rule_build_slab(dev.h, npt, 1, 3, L.WANT_EIG, C.byref(slab)))
    L.check(lib.abz_ptr_rule_build_slab(dev.h, npt, 1, 3, L.WANT_EIG, C.byref(halo)))
    L.check(lib.abz_rule_ltm_halo(halo))
    honly = abz.DeviceRule(dev, npt, None, L.WANT_H)
    for other, code in ((honly._h, L.ERR_ARG), (irr, L.ERR_UNSUPPORTED), (slab, L.ERR_UNSUPPORTED), (halo, L.ERR_UNSUPPORTED)):
        refused(f(other, pE, 3, L.LTM_STATES, pout), code)
        base, nb, ne = C.c_void_p(1), C.c_int64(-1), C.c_int(-1)
        assert lib.abz_rule_ltm_node_weights_ptr(other, C.byref(base), C.byref(nb), C.byref(ne)) == 0
        assert (base.value, nb.value, ne.value) == (None, 0, 0)
    assert b"not a whole periodic grid" in lib.abz_last_error()
    # valid calls afterwards still work and write their own results only
    assert f(h, pE, 3, L.LTM_STATES, pout) == 0
    got = out[:3 * 3 * npt ** 3].reshape(3, npt ** 3, 3)
    assert np.all(out[3 * 3 * npt ** 3:] == -99.0)
    check_nk(got, on_nodes(full, onw.node_weights(ln.rule_eigenvalues(full), Es, True)), npt ** 3, "a valid call after the refusals")
    assert np.abs(got - kept).max() * npt ** 3 > 1e-3  # the block is the optimized one now
    assert full.ltm_node_weights_ptr()[1:] == kept_ptr[1:]
    assert lib.abz_rule_destroy(irr) == 0 and lib.abz_rule_destroy(slab) == 0 and lib.abz_rule_destroy(halo) == 0


# ---------------------------------------------------------------- 10. lifetime and accounting
def test_optimized_node_weights_follow_the_rule(abz):
    s, rule = case_rule(abz, 3, 5)
    Es = np.array([0.1, 0.4, -0.2])
    rule.ltm_node_weights_optimized(Es)
    assert rule.ltm_node_weights_ptr()[1:] == (8 * 25 * 3 * 3 * 16, 3)
    rule.ltm_node_weights_optimized(Es[:1], states=False)
    assert rule.ltm_node_weights_ptr()[1:] == (8 * 25 * 1 * 3 * 16, 1)
    rule.rebuild()
    assert rule.ltm_node_weights_ptr() == (0, 0, 0)
    with pytest.raises(ValueError, match="holds no weights"):
        rule.ltm_node_weights_dot(np.ones((1, 125, 3)))


def books(L, ctx):
    info = (C.c_int64 * 5)()
    L.check(L.lib().abz_mem_info(ctx, info))
    return int(info[0]), int(info[4]), int(info[2])  # live bytes, live blocks, bytes of the context's scratch


def test_optimized_node_weights_are_accounted(abz):
    """abz_mem_info counts the block, 8 npt^2 nE n row bytes, as the rule's; the corner weights are the context's scratch and stay
    when the rule drops its weights; destroying everything gives everything back (the pattern of
    test_gpu_ltm_node_weights.py::test_node_weights_are_accounted, on a 3-d series)."""
    L = abz._lib
    lib = L.lib()
    npt, n, nE = 6, 2, 5
    rng = np.random.default_rng(6)
    c = rng.standard_normal((3, 3, 3, n, n)) + 1j * rng.standard_normal((3, 3, 3, n, n))
    c = np.ascontiguousarray(0.5 * (c + np.conj(np.swapaxes(c[::-1, ::-1, ::-1], -1, -2))))
    dims, first, per = np.array([3, 3, 3], dtype=np.int32), np.array([-1, -1, -1], dtype=np.int32), np.ones(3)
    Es = np.array([0.1, -0.3, 0.2, 0.0, 0.5])
    pE = Es.ctypes.data_as(L.c_f64p)
    block = 8 * npt ** 2 * nE * n * 16  # lines x energies x bands x padded row
    gc.collect()
    gc.disable()
    try:
        for attempt in range(2):  # the first round warms the allocator's pool: blocks, not bytes, could differ
            b0 = books(L, None)
            ctx, s, full = C.c_void_p(), C.c_void_p(), C.c_void_p()
            L.check(lib.abz_ctx_create(0, C.byref(ctx)))
            L.check(lib.abz_series_create(ctx, c.view(np.float64).ctypes.data_as(L.c_f64p), 3, dims.ctypes.data_as(L.c_i32p),
                                          first.ctypes.data_as(L.c_i32p), per.ctypes.data_as(L.c_f64p), n, C.byref(s)))
            L.check(lib.abz_ptr_rule_build(s, npt, 0, None, None, L.WANT_EIG, C.byref(full)))
            L.check(lib.abz_rule_ltm_node_weights_optimized(full, pE, nE, L.LTM_STATES, None))  # (the scratch exists from here on)
            bA = books(L, ctx)
            assert bA[2] >= 8 * 24 * n * 4 * npt ** 3  # a group of 4 energies, the whole grid in one slab
            base, nb, ne = C.c_void_p(), C.c_int64(-1), C.c_int(-1)
            L.check(lib.abz_rule_ltm_node_weights_ptr(full, C.byref(base), C.byref(nb), C.byref(ne)))
            assert (nb.value, ne.value) == (block, nE)
            L.check(lib.abz_rule_rebuild(full))  # drops the block, not the scratch
            bB = books(L, ctx)
            assert bB[1] == bA[1] - 1 and bB[2] >= bA[2]
            L.check(lib.abz_rule_ltm_node_weights_optimized(full, pE, nE, L.LTM_DOS, None))
            bC = books(L, ctx)  # (the allocator may hand out a cached block with more room: blocks are counted as they come)
            assert bC[1] == bB[1] + 1 and block <= bC[0] - bB[0] <= 2 * block and bC[2] == bB[2]  # the scratch was there already
            L.check(lib.abz_rule_ltm_node_weights_optimized(full, pE, nE, L.LTM_STATES, None))  # replaced, not added
            assert books(L, ctx)[1:] == bC[1:]
            assert lib.abz_rule_destroy(full) == 0  # with the weights resident
            assert lib.abz_series_destroy(s) == 0
            assert lib.abz_ctx_destroy(ctx) == 0
            b5 = books(L, None)
            print(f"books (live bytes, live blocks, scratch): start {b0}, weights {bA}, rebuilt {bB}, weights again {bC}, end {b5}")
            if attempt == 1:
                assert b5[:2] == b0[:2]
    finally:
        gc.enable()


# ---------------------------------------------------------------- 11. profiling
def test_optimized_node_weight_launches_are_profiled(abz):
    """One ProfScope of ABZ_K_LTM around the launches of a call, whatever the number of groups and slabs."""
    L = abz._lib
    s, rule = case_rule(abz, 3, 8)
    dev = s.device()
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        dev.ctx.prof_reset()
        rule.ltm_node_weights_optimized(np.linspace(-3, 3, 16), export=False)
        ms, launches = dev.ctx.prof_read(L.K_LTM)
        assert launches == 1 and ms > 0.0
        rule.ltm_node_weights_optimized(np.linspace(-3, 3, 5), states=False, export=False)
        assert dev.ctx.prof_read(L.K_LTM)[1] == 2
        assert dev.ctx.prof_read(L.K_GGR)[1] == 0
    finally:
        dev.ctx.prof_enable(False)

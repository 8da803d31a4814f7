"""Complex integration weights W_b(k; z) of the Green's function on the device (abz_rule_ltm_green_node_weights, _ptr, _dot,
_fold, _matrix; ltm_green_nodew_kernel of kernels_ltm_green_nodew.hip; DeviceRule.ltm_green_node_weights*, dos.green_weights,
dos.green_local_fused) against the scatter-form restatement of tests/gnodew_numpy.py, against the shipped scans and the
projector route, and their exact values, repeatability, lifetime, independence of the real weights, and refusals.

Parity bound: the restatement is fed the rule's own exported eigenvalues, so only summation order, FMA contraction and libm
remain.  A node weight is a sum of at most 24 corner weights of the kind the scans sum, of size 1 / nk: the bound of
test_gpu_ltm_node_weights.py on the O(1) quantity nk W,   |nk W - nk ref| <= 1e-9 max(1, max|nk ref|).  Against the shipped
scans (sums of the weights, contractions with elements): the scans' own bound 1e-9 max(1, max|ref|) on the real and the
imaginary part.  A value inside a call of 8 against the same value alone: 1e-13 max(1, max|nk W|), the bound of
test_gpu_ltm_density_matrix.py for multi-energy calls (another instantiation of the same arithmetic).

Shapes: those of test_gpu_ltm_node_weights.py -- npt = 2 (k + 1 and k - 1 are the same node), 3, odd sizes, a 1-D line longer
than a wave (65, row padded to 80), 2 and 3 variables, one and several bands, 6 and 33 bands.  Matrix: the shapes of
test_gpu_ltm_density_matrix.py that reach every path of its kernels."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import abz_oracle as orc
import gloc_ltm_numpy as gl
import gnodew_numpy as gnw
import ltm_numpy as ln
import unfold_numpy as un
import test_gpu_mem_books as mb
from test_gpu_ltm import product_series
from test_gpu_ltm_density_matrix import make_series as matrix_series
from test_gpu_ltm_green import close
from test_gpu_ltm_green_matrix import bits
from test_gpu_ltm_node_weights import CASES, read_block, series_of
from test_gpu_parity import rand_series
from test_ltm_unfold_cpu import model_sym_sets

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def z_list(eig):
    """12 values: inside the bands at Im z = 1e-2, 1e-4, 1e-6, 0.5 and -1e-2; below and above the bands; the band edges, a node's
    own eigenvalue and the Gamma eigenvalues at +1e-8j (narrow sub-ranges and the Taylor branch)."""
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo if hi > lo else 1.0
    gamma = eig[(0,) * (eig.ndim - 1)]
    flat = eig.reshape(-1)
    t = lo + w * np.array([0.37, 0.52, 0.71, 0.13])
    return np.array([t[0] + 1e-2j, t[1] + 1e-4j, t[2] + 1e-6j, t[3] + 0.5j, t[0] - 1e-2j, lo - 0.3 * w + 1e-3j, hi + 0.3 * w + 0.2j,
                     lo + 1e-8j, hi + 1e-8j, flat[(7 * len(flat)) // 11] + 1e-8j, gamma[0] + 1e-8j, gamma[-1] + 1e-8j])


# the calls of 1, 3 and 8 values (in one and two variables a single launch; a pair and a single one; four pairs -- in three every
# value is a launch of its own): positions in z_list, in no order, the 8 with one value twice
CALLS = {1: [2], 3: [9, 4, 7], 8: [11, 8, 5, 3, 1, 6, 1, 0]}


def close_nk(u, ref, nk):
    """(deviation, bound) of the parity check on nk W, on the real and the imaginary part"""
    u, ref = nk * np.asarray(u), nk * np.asarray(ref)
    dev = max(float(np.abs(u.real - ref.real).max()), float(np.abs(u.imag - ref.imag).max()))
    return dev, 1e-9 * max(1.0, float(np.abs(ref.real).max()), float(np.abs(ref.imag).max()))


def check_nk(u, ref, nk, what):
    assert u.shape == ref.shape and u.dtype == np.complex128 and np.all(np.isfinite(bits(u))), (what, u.shape, ref.shape)
    dev, bound = close_nk(u, ref, nk)
    print(f"green nodew {what}: max dev of nk W {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)
    return dev / bound


def check(u, ref, what):
    u, ref = np.asarray(u), np.asarray(ref)
    assert u.shape == ref.shape and np.all(np.isfinite(bits(u.astype(np.complex128)))), (what, u.shape, ref.shape)
    dev, bound = close(u, ref)
    print(f"green nodew {what}: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)


def on_nodes(rule, Wgrid):
    """restatement weights [nz] + [npt]*d + [n] -> [nz, nk, n], the order of the export"""
    return Wgrid.reshape(Wgrid.shape[0], rule.nk, Wgrid.shape[-1])


def read_gblock(abz, rule):
    """The resident complex block through ltm_green_node_weights_ptr and hipMemcpy: [ntiles, 2 nz n planes, row]"""
    L = abz._lib
    base, nbytes, nz = rule.ltm_green_node_weights_ptr()
    assert base and nbytes > 0 and nz > 0
    n, d, npt = rule.dev.s.n, rule.dev.s.d, rule.npt
    row = (npt + 15) // 16 * 16
    assert nbytes == 8 * npt ** (d - 1) * 2 * nz * n * row
    buf = np.empty(nbytes // 8)
    memcpy = L.lib().hipMemcpy  # (the HIP runtime the library is linked against)
    memcpy.restype, memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert memcpy(buf.ctypes.data, base, nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return buf.reshape(npt ** (d - 1), 2 * nz * n, row)


_SHARED = {}


def shared(abz, name, npt):
    """Per case, made once and left unchanged: the rule, its eigenvalues, the 12 values of z and the restatement's weights"""
    key = (name, npt)
    if key not in _SHARED:
        rule = series_of(abz, name).device().rule(npt, None, abz._lib.WANT_EIG)
        eig = ln.rule_eigenvalues(rule)
        zs = z_list(eig)
        ref = on_nodes(rule, gnw.node_weights(eig, zs))
        ref.setflags(write=False)
        _SHARED[key] = dict(rule=rule, eig=eig, zs=zs, ref=ref, n=eig.shape[-1])
    return _SHARED[key]


# ---------------------------------------------------------------- 1. parity with the restatement
@pytest.mark.parametrize("name,npt", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_green_node_weights_match_restatement(abz, name, npt):
    sh = shared(abz, name, npt)
    rule, zs, ref, n = sh["rule"], sh["zs"], sh["ref"], sh["n"]
    worst = 0.0
    for nz, pick in CALLS.items():
        W = rule.ltm_green_node_weights(zs[pick])
        assert W.shape == (nz, rule.nk, n)
        worst = max(worst, check_nk(W, ref[pick], rule.nk, f"{name} npt={npt} nz={nz}"))
        assert rule.ltm_green_node_weights_ptr()[2] == nz
    print(f"green nodew parity {name} npt={npt}: worst deviation / bound = {worst:.3e}")


# ---------------------------------------------------------------- 2. against the shipped scans
@pytest.mark.parametrize("name,npt", [("chain2", 65), ("int2", 17), ("svo", 6), ("syn6", 5)])
def test_green_node_weights_against_the_shipped_scans(abz, name, npt):
    sh = shared(abz, name, npt)
    rule, zs, eig, n = sh["rule"], sh["zs"], sh["eig"], sh["n"]
    A = np.random.default_rng(2).standard_normal((16, rule.nk, n))
    rule.ltm_elements(A)
    tr = rule.ltm_green(zs)
    scan = rule.ltm_green(zs, elements="attached")  # [12, 16]
    energy = rule.ltm_green(zs, elements="energy")[:, 0]
    e = eig.reshape(rule.nk, n)
    for nz, pick in CALLS.items():
        W = rule.ltm_green_node_weights(zs[pick])
        check(W.sum(axis=(1, 2)), tr[pick], f"{name} nz={nz} sum of the weights against tr G")
        check(np.einsum("zkb,ckb->zc", W, A), scan[pick], f"{name} nz={nz} einsum(W, A) against the scan")
        dot = rule.ltm_green_node_weights_dot()
        assert dot.shape == (nz, 16) and dot.dtype == np.complex128
        check(dot, scan[pick], f"{name} nz={nz} dot against the scan")
        check(np.einsum("zkb,kb->z", W, e), energy[pick], f"{name} nz={nz} einsum(W, e) against elements='energy'")
    # an array attaches first and leaves the weights in place; fewer components than 16
    few = rule.ltm_green_node_weights_dot(A[:3])
    check(few, scan[CALLS[8]][:, :3], f"{name} dot of 3 components")
    rule.ltm_elements(None)
    assert rule.ltm_green_node_weights_ptr()[2] == 8  # dropping ELEMENTS leaves the weights alone


# ---------------------------------------------------------------- 3. exact values
@pytest.mark.parametrize("d,npt", [(1, 2), (1, 65), (2, 5), (3, 3)])
def test_flat_band_weighs_every_node_alike(abz, d, npt):
    """A one-band series with the constant e0: every corner weight is 1 / ((d+1) u), so nk W = 1 / (z - e0): within 4 eps
    relative."""
    e0 = 0.25
    c = np.zeros((3,) * d + (1, 1), dtype=np.complex128)
    c[(1,) * d] = e0
    rule = abz.FourierSeries(c, period=1.0, first=(-1,) * d, ndim=d).device().rule(npt, None, abz._lib.WANT_EIG)
    assert np.all(ln.rule_eigenvalues(rule) == e0)
    zs = np.array([e0 + 1e-8j, e0 + 0.3 - 1e-2j, -4.0 + 0.5j, e0 - 1e-6j, 7.0 + 1e-4j])
    W = rule.ltm_green_node_weights(zs)
    for i, z in enumerate(zs):
        ref = 1.0 / (z - e0)
        dev = float(np.abs(rule.nk * W[i] - ref).max()) / abs(ref)
        print(f"flat band d={d} npt={npt} z={z}: |nk W - 1 / (z - e0)| = {dev / EPS:.2f} eps relative")
        assert dev <= 4 * EPS


# ---------------------------------------------------------------- 4. conjugation, repeatability, padding, groups
@pytest.mark.parametrize("name,npt", [("chain2", 65), ("int2", 5), ("svo", 6)])
def test_green_node_weights_conjugate_repeat_and_pad(abz, name, npt):
    sh = shared(abz, name, npt)
    rule, zs, n = sh["rule"], sh["zs"], sh["n"]
    d = rule.dev.s.d
    rule.ltm_elements(np.random.default_rng(4).standard_normal((5, rule.nk, n)))
    for pick in CALLS.values():
        a = rule.ltm_green_node_weights(zs[pick])
        da = rule.ltm_green_node_weights_dot()
        block_a = read_gblock(abz, rule)
        b = rule.ltm_green_node_weights(zs[pick])
        db = rule.ltm_green_node_weights_dot()
        block = read_gblock(abz, rule)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(da), bits(db)) and np.array_equal(block_a, block)
        assert np.all(block[:, :, npt:] == 0.0) and not np.any(np.signbit(block[:, :, npt:]))  # the padding columns
        # the block is the export: plane (2 i + part) n + b of line l, column c = Re / Im W_b(k = l npt + c; z_i)
        got = block[:, :, :npt].reshape(npt ** (d - 1), len(pick), 2, n, npt).transpose(1, 0, 4, 3, 2).reshape(len(pick), rule.nk, n, 2)
        assert np.array_equal(np.ascontiguousarray(got).view(np.complex128)[..., 0], b)
        # W(conj z) is conj W(z), to the bit
        c = rule.ltm_green_node_weights(np.conj(zs[pick]))
        assert np.array_equal(bits(c), bits(np.conj(a)))
        assert np.array_equal(bits(rule.ltm_green_node_weights_dot()), bits(np.conj(da)))
    assert rule.ltm_green_node_weights(zs[:5], export=False) is None and rule.ltm_green_node_weights_ptr()[2] == 5
    rule.ltm_elements(None)
    # a value inside a call of 8 against the same value alone
    W8 = rule.ltm_green_node_weights(zs[CALLS[8]])
    scale = max(1.0, float(np.abs(rule.nk * W8).max()))
    for j, i in enumerate(CALLS[8]):
        W1 = rule.ltm_green_node_weights(zs[i:i + 1])[0]
        dev = float(np.abs(rule.nk * (W8[j] - W1)).max())
        print(f"{name} npt={npt}: z[{i}] inside a call of 8 against alone: nk |dW| = {dev:.2e} (bound {1e-13 * scale:.1e})")
        assert dev <= 1e-13 * scale


# ---------------------------------------------------------------- 5. unfolded rules
@pytest.mark.parametrize("name,npt,d", [("svo", 6, 3), ("int2", 8, 2)])
def test_green_node_weights_of_an_unfolded_rule_and_their_fold(abz, name, npt, d):
    L = abz._lib
    s = series_of(abz, name)
    dev = s.device()
    syms = model_sym_sets(abz, name, d)["cubic"]
    src = abz.DeviceRule(dev, npt, syms, L.WANT_EIG)
    unf = src.unfold()
    full = dev.rule(npt, None, L.WANT_EIG)
    eig = ln.rule_eigenvalues(unf)
    n, nk, nirr = eig.shape[-1], unf.nk, src.nk
    zs = z_list(eig)[CALLS[8]]
    se = src.export(eig=True)
    node_of = un.orbit_map(npt, d, syms, se["x"])  # the orbits on the host, from the exported nodes and the matrices
    W = unf.ltm_green_node_weights(zs)
    check_nk(W, full.ltm_green_node_weights(zs), nk, f"{name} npt={npt} unfolded against the full build")
    ref = on_nodes(unf, gnw.node_weights(eig, zs))
    check_nk(W, ref, nk, f"{name} npt={npt} unfolded against the restatement")
    fold = unf.ltm_green_node_weights_fold()
    assert fold.shape == (len(zs), nirr, n) and fold.dtype == np.complex128
    host = np.zeros_like(fold)
    np.add.at(host, (slice(None), node_of), W)
    # an orbit holds at most 48 points: the bound on nk W, for sums of up to 48 of them
    check_nk(fold, host, nk, f"{name} npt={npt} fold against host orbit sums of the export")
    assert np.array_equal(bits(fold), bits(unf.ltm_green_node_weights_fold()))  # no atomics: the same bits
    # A = e^2 is exactly symmetric (unfolded eigenvalues are copies): folded sum on the irreducible nodes = full-grid dot
    A = np.square(unf.export(x=False, w=False, eig=True)["eig"])[None]
    dot = unf.ltm_green_node_weights_dot(A)[:, 0]
    check(np.einsum("zjb,jb->z", fold, np.square(se["eig"])), dot, f"{name} npt={npt} folded sum of e^2 against the full-grid dot")
    unf.ltm_elements(None)
    # a new gather drops the block
    unf.rebuild()
    assert unf.ltm_green_node_weights_ptr() == (0, 0, 0)
    with pytest.raises(ValueError, match="holds no weights"):
        unf.ltm_green_node_weights_fold()


# ---------------------------------------------------------------- 6. the matrix G_pq(z)
MATRIX = ["syn2_5", "syn3_5", "syn4_5", "rand5_40", "rand9_17", "syn17_5", "syn32_3", "svo_8"]


def matrix_z(eig):
    lo, hi = float(eig.min()), float(eig.max())
    w = hi - lo
    return np.array([lo + 0.37 * w + 1e-2j, lo + 0.6 * w - 0.3j, lo + 0.52 * w + 1e-4j, hi + 0.2 * w + 1e-6j, lo + 0.37 * w + 1e-2j,
                     lo + 0.1 * w + 0.5j, lo + 0.8 * w - 1e-3j, float(eig.reshape(-1)[eig.size // 3]) + 1e-8j, lo - 0.5 * w + 0.1j])


@pytest.mark.parametrize("name", MATRIX)
def test_green_matrix_from_the_node_weights(abz, name):
    L = abz._lib
    s, npt = matrix_series(abz, name)
    rule = abz.DeviceRule(s.device(), npt, None, L.WANT_H | L.WANT_EIG)
    eig = ln.rule_eigenvalues(rule)
    n = eig.shape[-1]
    zs = matrix_z(eig)  # 9 values: a chunk of 8 and one more
    G = rule.ltm_green_node_weights_matrix(zs)
    assert G.shape == (len(zs), n, n) and G.dtype == np.complex128 and np.all(np.isfinite(bits(G)))
    assert rule.ltm_green_node_weights_ptr()[2] == 1  # the last chunk stays resident
    # the projector route: same solver, same basis
    check(G, rule.ltm_green_matrix(zs), f"matrix {name} against ltm_green_matrix")
    rule.ltm_elements(None)
    # LAPACK's projectors of the exported H (generic series: no degenerate levels)
    if name != "svo_8":
        H = rule.export(x=False, w=False, H=True)["H"].reshape(eig.shape[:-1] + (n, n))
        few = zs[:2] if n >= 17 else zs[:4]
        check(G[:len(few)], gl.green_matrix(eig, H, few), f"matrix {name} against the restatement with LAPACK's projectors")
    # the diagonal: orbital weights through the weighted scan (at most 16 components); the trace: tr G
    orb = list(range(min(n, 16)))
    rule.ltm_orbitals(orb)
    check(np.einsum("zpp->zp", G)[:, :len(orb)], rule.ltm_green(zs, elements="attached"), f"matrix {name} diagonal against orbital weights")
    rule.ltm_elements(None)
    check(np.trace(G, axis1=1, axis2=2), rule.ltm_green(zs), f"matrix {name} trace against tr G")
    # G(z)^dagger = G(conj z), to the bit (W(conj z) = conj W(z) to the bit, X and Y Hermitian to the bit); two calls, same bits
    Gc = rule.ltm_green_node_weights_matrix(np.conj(zs))
    assert np.array_equal(bits(np.conj(G.transpose(0, 2, 1))), bits(Gc))
    assert np.array_equal(bits(G), bits(rule.ltm_green_node_weights_matrix(zs)))
    assert n == 1 or np.abs(G - np.conj(G.transpose(0, 2, 1))).max() > 0.0  # not Hermitian
    # a selection of orbitals is the sub-block, in the order asked for; the resident weights without zs
    sel = [n - 1, 0]
    assert np.array_equal(bits(rule.ltm_green_node_weights_matrix(zs, orbitals=sel)), bits(G[:, sel][:, :, sel]))
    assert np.array_equal(bits(rule.ltm_green_node_weights_matrix()), bits(G[8:]))
    rule.close()


@pytest.mark.parametrize("name", ["syn3_5", "rand9_17"])
def test_green_matrix_does_not_depend_on_the_h_source(abz, name):
    L = abz._lib
    s, npt = matrix_series(abz, name)
    got = []
    for want in (L.WANT_H | L.WANT_EIG, L.WANT_H | L.WANT_EIG | L.WANT_H_COMPACT, L.WANT_EIG):  # full, compact, transient
        rule = abz.DeviceRule(s.device(), npt, None, want)
        if not got:
            zs = matrix_z(ln.rule_eigenvalues(rule))[:8]
        A = np.random.default_rng(8).standard_normal((2, rule.nk, s.n))
        rule.ltm_elements(A)
        got.append(rule.ltm_green_node_weights_matrix(zs))
        assert rule._ltm_ncomp == 2 and np.array_equal(rule.ltm_elements_export(), A)  # nothing was attached
        rule.close()
    assert np.array_equal(bits(got[0]), bits(got[1])) and np.array_equal(bits(got[0]), bits(got[2]))


def test_green_local_fused_against_the_default(abz):
    h = abz.load_w90_series(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svo_hr.dat.gz"))
    bz = abz.load_bz(abz.FBZ(), 3.85856 * np.eye(3))
    eig0 = ln.rule_eigenvalues(h.device().rule(8, None, abz._lib.WANT_EIG))
    zs = np.linspace(eig0.min() - 0.1, eig0.max() + 0.1, 11) + 1e-2j
    cache = abz.dos.init(abz.DOSProblem(h, 0.0, bz), abz.LTM(npt=8))
    G = abz.dos.green_local(cache, zs)
    F = abz.dos.green_local_fused(cache, zs)
    check(F, G, "green_local_fused against green_local")
    assert np.array_equal(bits(abz.dos.green_local_fused(cache, zs, orbitals=[2, 0])), bits(F[:, [2, 0]][:, :, [2, 0]]))
    assert np.array_equal(bits(abz.dos.green_local(cache, zs)), bits(G))  # the default route: its own bits, before and after
    Fp = abz.dos.green_local_fused(abz.DOSProblem(h, 0.0, bz), zs[:2])
    assert Fp.shape == (2, 3, 3)
    # the weights of the front end: a scalar, a list, and the fold of a symmetric cache
    W1, z1 = abz.dos.green_weights(cache, zs[3])
    assert W1.shape == (cache.cacheval.nk, 3) and z1 == zs[3]
    Wl, zl = abz.dos.green_weights(cache, zs[:3])
    assert Wl.shape == (3, cache.cacheval.nk, 3) and np.array_equal(zl, zs[:3])
    check(Wl.sum(axis=(1, 2)), abz.dos.green_trace(cache, zs[:3]), "green_weights sum to green_trace")
    cub = abz.load_bz(abz.CubicSymIBZ(), 3.85856 * np.eye(3))
    csym = abz.dos.init(abz.DOSProblem(h, 0.0, cub), abz.LTM(npt=8, symmetric=True))
    Wf, _ = abz.dos.green_weights(csym, zs[:3], fold=True)
    src = csym.cacheval.source
    assert Wf.shape == (3, src.nk, 3)
    check(np.einsum("zjb,jb->z", Wf, src.export(x=False, w=False, eig=True)["eig"]), cache.cacheval.ltm_green(zs[:3], elements="energy")[:, 0],
          "folded weights times e against the full-grid scan with elements='energy'")
    with pytest.raises(ValueError, match="fold=True"):
        abz.dos.green_weights(cache, zs[:3], fold=True)
    with pytest.raises(ValueError, match="symmetric=False"):
        abz.dos.green_local_fused(csym, zs[:3])


# ---------------------------------------------------------------- 7. independence of the real weights, lifetime, books
def test_real_and_complex_weights_do_not_touch_each_other(abz):
    sh = shared(abz, "svo", 6)
    rule, zs, n = sh["rule"], sh["zs"], sh["n"]
    Es = np.array([12.3, 12.9, 12.6])
    rule.ltm_elements(np.random.default_rng(12).standard_normal((3, rule.nk, n)))
    Wr = rule.ltm_node_weights(Es)
    dr, pr, br = rule.ltm_node_weights_dot(), rule.ltm_node_weights_ptr(), read_block(abz, rule)
    Wc = rule.ltm_green_node_weights(zs[CALLS[3]])
    dc, pc, bc = rule.ltm_green_node_weights_dot(), rule.ltm_green_node_weights_ptr(), read_gblock(abz, rule)
    assert rule.ltm_node_weights_ptr() == pr and np.array_equal(read_block(abz, rule), br) and np.array_equal(rule.ltm_node_weights_dot(), dr)
    # real calls in between leave the complex block alone, and give their own bits again
    assert np.array_equal(rule.ltm_node_weights(Es), Wr) and np.array_equal(rule.ltm_node_weights_dot(), dr)
    rule.ltm_node_weights(Es[:1], states=False, export=False)
    assert rule.ltm_green_node_weights_ptr() == pc and np.array_equal(read_gblock(abz, rule), bc)
    assert np.array_equal(bits(rule.ltm_green_node_weights_dot()), bits(dc))
    # and the reverse
    rule.ltm_node_weights(Es, export=False)
    pr = rule.ltm_node_weights_ptr()
    assert np.array_equal(bits(rule.ltm_green_node_weights(zs[CALLS[3]])), bits(Wc))
    rule.ltm_green_node_weights(zs[CALLS[8]], export=False)
    assert rule.ltm_node_weights_ptr() == pr and np.array_equal(read_block(abz, rule), br) and np.array_equal(rule.ltm_node_weights_dot(), dr)
    rule.ltm_elements(None)
    assert rule.ltm_green_node_weights_ptr()[2] == 8 and rule.ltm_node_weights_ptr()[2] == 3


def test_green_node_weights_follow_the_rule(abz):
    """Dropped by a rebuild and by an update of the series (the old eigenvalues are gone), replaced by the next call."""
    from test_gpu_ltm_node_weights import two_band_chain
    s = two_band_chain(abz)
    rule = s.device().rule(9, None, abz._lib.WANT_EIG)
    zs = np.array([0.1 + 1e-2j, 0.4 - 0.3j, -0.2 + 1e-5j])
    rule.ltm_green_node_weights(zs)
    assert rule.ltm_green_node_weights_ptr()[1:] == (8 * 2 * 3 * 2 * 16, 3)
    rule.ltm_green_node_weights(zs[:1])
    assert rule.ltm_green_node_weights_ptr()[1:] == (8 * 2 * 1 * 2 * 16, 1)
    rule.rebuild()
    assert rule.ltm_green_node_weights_ptr() == (0, 0, 0)
    with pytest.raises(ValueError, match="holds no weights"):
        rule.ltm_green_node_weights_dot(np.ones((1, 9, 2)))
    with pytest.raises(ValueError, match="holds no weights"):
        rule.ltm_green_node_weights_matrix()
    W1 = rule.ltm_green_node_weights(zs)
    s.c *= 1.5
    s.invalidate()
    assert rule.ltm_green_node_weights_ptr() == (0, 0, 0)
    W2 = rule.ltm_green_node_weights(1.5 * zs)  # G of 1.5 H at 1.5 z is G / 1.5
    check_nk(1.5 * W2, W1, 9, "weights of the scaled series at the scaled z")


def test_green_node_weights_are_accounted(abz):
    """abz_mem_info counts the block; a replacement does not add one; a rebuild drops it; a matrix call with its transient H-only
    rule leaves nothing behind; destroying the rules and the series gives everything back (the pattern of test_gpu_mem_books.py)."""
    L = abz._lib
    lib = L.lib()
    gc.collect()
    gc.disable()
    try:
        for attempt in range(2):  # the first round warms the allocator's pool: blocks, not bytes, could differ
            b0 = mb.books(L, None)
            ctx = mb.create_ctx(L)
            s = mb.create_series(L, ctx, 2, seed=6)
            full = mb.build_full(L, s, L.WANT_EIG)
            zs = np.array([0.1 + 0.1j, -0.3 - 0.2j, 0.2 + 1e-3j])
            pz = zs.view(np.float64).ctypes.data_as(L.c_f64p)
            G = np.zeros((3, 2, 2), dtype=np.complex128)
            pG = G.view(np.float64).ctypes.data_as(L.c_f64p)
            b1 = mb.books(L, ctx)
            L.check(lib.abz_rule_ltm_green_node_weights(full, pz, 3, None))
            b2 = mb.books(L, ctx)
            block = 8 * mb.NPT * 2 * 3 * 2 * 16  # lines x (re, im) x values x bands x padded row
            assert b2[0] - b1[0] >= block and b2[1] == b1[1] + 1
            L.check(lib.abz_rule_ltm_green_node_weights(full, pz, 3, None))  # replaced, not added
            b2b = mb.books(L, ctx)
            assert b2b[1] == b2[1] and block <= b2b[0] - b1[0] <= 2 * block
            L.check(lib.abz_rule_ltm_green_node_weights_matrix(full, pG))  # the scratch of the sums and of the transient rule exists from here on
            b3 = mb.books(L, ctx)
            L.check(lib.abz_rule_ltm_green_node_weights_matrix(full, pG))
            assert mb.books(L, ctx) == b3
            L.check(lib.abz_rule_rebuild(full))  # drops the block
            assert mb.books(L, ctx)[1] == b3[1] - 1
            L.check(lib.abz_rule_ltm_green_node_weights(full, pz, 3, None))
            mb.destroy(L, full)  # with the weights resident
            assert lib.abz_series_destroy(s) == 0
            assert lib.abz_ctx_destroy(ctx) == 0
            b5 = mb.books(L, None)
            print(f"books (live bytes, live blocks): start {b0}, rule {b1}, weights {b2}, after the matrix {b3}, end {b5}")
            if attempt == 1:
                assert b5 == b0
    finally:
        gc.enable()


# ---------------------------------------------------------------- 8. refusals
def test_green_node_weight_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s = product_series(abz, orc.synthetic_wannier(3, rmax=2, seed=7))
    dev = s.device()
    npt = 4
    nk = npt ** 3
    zs = np.array([0.5 + 0.1j, 1.5 - 1e-3j, -0.5 + 1e-6j])
    Es = np.array([0.5, 1.5])
    pz = zs.view(np.float64).ctypes.data_as(L.c_f64p)
    out = np.full(2 * 9 * nk * 3 + 2 * 8 * 33 * 33, -99.0)
    pout = out.ctypes.data_as(L.c_f64p)
    full = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    h = full._h
    A = np.random.default_rng(2).standard_normal((2, nk, 3))
    full.ltm_elements(A)
    kept = full.ltm_green_node_weights(zs)
    full.ltm_node_weights(Es, export=False)

    def state(rule):
        pc, pr = rule.ltm_green_node_weights_ptr(), rule.ltm_node_weights_ptr()
        return (pc, read_gblock(abz, rule) if pc[2] else None, pr, read_block(abz, rule) if pr[2] else None, rule.ltm_elements_export())

    def same(a, b):
        return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))

    def refused(rule, before, rc, code, words=None):
        msg = lib.abz_last_error().decode()
        assert rc == code and len(msg) > 0, (rc, code, msg)
        assert words is None or words in msg, msg
        assert np.all(out == -99.0)  # nothing was written
        # both weight blocks (pointer, size, contents) and the attached elements are what they were
        assert same(state(rule), before), msg

    st = state(full)
    f64 = lambda a: np.ascontiguousarray(a).view(np.float64).ctypes.data_as(L.c_f64p)
    # the arguments of the gather
    refused(full, st, lib.abz_rule_ltm_green_node_weights(h, None, 3, pout), L.ERR_ARG, "null z")
    for nz in (0, 9, -1):
        refused(full, st, lib.abz_rule_ltm_green_node_weights(h, pz, nz, pout), L.ERR_ARG, "outside 1..8")
    refused(full, st, lib.abz_rule_ltm_green_node_weights(h, f64(np.array([0.5 + 0.1j, 0.7 + 0j])), 2, pout), L.ERR_ARG, "is real")
    for bad in (np.nan + 0.1j, 0.1 + 1j * np.inf, complex(np.inf, 0.1)):
        refused(full, st, lib.abz_rule_ltm_green_node_weights(h, f64(np.array([0.5 + 0.1j, bad])), 2, pout), L.ERR_ARG, "not finite")
    for fn in (lib.abz_rule_ltm_green_node_weights_dot, lib.abz_rule_ltm_green_node_weights_fold, lib.abz_rule_ltm_green_node_weights_matrix):
        refused(full, st, fn(h, None), L.ERR_ARG, "null out")
    refused(full, st, lib.abz_rule_ltm_green_node_weights_fold(h, pout), L.ERR_ARG, "not made by abz_rule_ltm_unfold")
    # rules that are not a whole periodic grid, or hold no eigenvalues
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, npt, cub.syms, L.WANT_EIG)
    idx, w = abz.symptr_rule(npt, 3, cub.syms)
    irr, slab, halo = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, npt, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(irr)))
    L.check(lib.abz_ptr_rule_build_slab(dev.h, npt, 1, 3, L.WANT_EIG, C.byref(slab)))
    L.check(lib.abz_ptr_rule_build_slab(dev.h, npt, 1, 3, L.WANT_EIG, C.byref(halo)))
    L.check(lib.abz_rule_ltm_halo(halo))
    honly = abz.DeviceRule(dev, npt, None, L.WANT_H)
    for other, code in ((honly._h, L.ERR_ARG), (sym._h, L.ERR_UNSUPPORTED), (irr, L.ERR_UNSUPPORTED), (slab, L.ERR_UNSUPPORTED),
                        (halo, L.ERR_UNSUPPORTED)):
        refused(full, st, lib.abz_rule_ltm_green_node_weights(other, pz, 3, pout), code)
        refused(full, st, lib.abz_rule_ltm_green_node_weights_dot(other, pout), code)
        refused(full, st, lib.abz_rule_ltm_green_node_weights_fold(other, pout), code)
        refused(full, st, lib.abz_rule_ltm_green_node_weights_matrix(other, pout), code)
        base, nb, nz = C.c_void_p(1), C.c_int64(-1), C.c_int(-1)
        assert lib.abz_rule_ltm_green_node_weights_ptr(other, C.byref(base), C.byref(nb), C.byref(nz)) == 0
        assert (base.value, nb.value, nz.value) == (None, 0, 0)
    assert b"not a whole periodic grid" in lib.abz_last_error()
    assert lib.abz_rule_destroy(irr) == 0 and lib.abz_rule_destroy(slab) == 0 and lib.abz_rule_destroy(halo) == 0
    honly.close()
    # no resident complex weights (real ones and elements are there): dot, matrix; fold on an unfolded rule
    other = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    other.ltm_elements(A)
    other.ltm_node_weights(Es, export=False)
    so = state(other)
    refused(other, so, lib.abz_rule_ltm_green_node_weights_dot(other._h, pout), L.ERR_ARG, "holds no complex integration weights")
    refused(other, so, lib.abz_rule_ltm_green_node_weights_matrix(other._h, pout), L.ERR_ARG, "holds no complex integration weights")
    # complex weights, nothing attached
    other.ltm_elements(None)
    other.ltm_green_node_weights(zs, export=False)
    refused(other, state(other), lib.abz_rule_ltm_green_node_weights_dot(other._h, pout), L.ERR_ARG, "no matrix elements")
    other.close()
    unf = sym.unfold()
    unf.ltm_elements(np.ones((1, nk, 3)))
    unf.ltm_node_weights(Es, export=False)
    su = state(unf)
    refused(unf, su, lib.abz_rule_ltm_green_node_weights_fold(unf._h, pout), L.ERR_ARG, "holds no complex integration weights")
    with pytest.raises(ValueError, match="holds no weights"):
        unf.ltm_green_node_weights_fold()
    # an unfolded rule holds complex weights, but no H(k)
    unf.ltm_green_node_weights(zs, export=False)
    refused(unf, state(unf), lib.abz_rule_ltm_green_node_weights_matrix(unf._h, pout), L.ERR_UNSUPPORTED, "unfolded")
    unf.close()
    sym.close()
    # 33 bands: the weights work, the matrix has no kernel
    sn = product_series(abz, orc.synthetic_wannier(33, rmax=2, seed=7))
    r33 = abz.DeviceRule(sn.device(), 3, None, L.WANT_EIG)
    r33.ltm_elements(np.ones((1, r33.nk, 33)))
    assert r33.ltm_green_node_weights(zs).shape == (3, 27, 33)
    r33.ltm_node_weights(Es, export=False)
    refused(r33, state(r33), lib.abz_rule_ltm_green_node_weights_matrix(r33.h, pout), L.ERR_UNSUPPORTED, "33 bands")
    r33.close()
    # a series that is not Hermitian
    c, first = rand_series(np.random.default_rng(9), (3, 3, 3), 3, hermitian=False)
    rn = abz.DeviceRule(abz.FourierSeries(c, period=1.0, first=first).device(), npt, None, L.WANT_H | L.WANT_EIG)
    rn.ltm_elements(np.ones((1, rn.nk, 3)))
    rn.ltm_green_node_weights(zs, export=False)
    rn.ltm_node_weights(Es, export=False)
    refused(rn, state(rn), lib.abz_rule_ltm_green_node_weights_matrix(rn.h, pout), L.ERR_ARG, "Hermitian")
    rn.close()
    # valid calls afterwards still work, and write what they should and no more
    assert lib.abz_rule_ltm_green_node_weights(h, pz, 3, pout) == 0
    m = 2 * 3 * nk * 3
    assert np.array_equal(out[:m].view(np.complex128).reshape(3, nk, 3), kept) and np.all(out[m:] == -99.0)
    out[:] = -99.0
    assert lib.abz_rule_ltm_green_node_weights_dot(h, pout) == 0
    assert np.array_equal(out[:2 * 3 * 2].view(np.complex128).reshape(3, 2), full.ltm_green_node_weights_dot()) and np.all(out[12:] == -99.0)
    out[:] = -99.0
    assert lib.abz_rule_ltm_green_node_weights_matrix(h, pout) == 0
    assert np.array_equal(bits(out[:2 * 3 * 9].view(np.complex128).reshape(3, 3, 3)), bits(full.ltm_green_node_weights_matrix()))
    assert np.all(out[54:] == -99.0)
    # (the valid gather replaced the complex block by one with the same contents; everything else is where it was)
    end = state(full)
    assert end[0][1:] == st[0][1:] and same(end[1:], st[1:])
    # the Python mirror refuses a k-sharded rule
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        r = dev.rule(npt, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError, match="halo"):
            r.ltm_green_node_weights(zs)
    finally:
        dev.kshard, dev.allreduce = None, None


# ---------------------------------------------------------------- profiling
def test_green_node_weight_launches_are_profiled(abz):
    """One ProfScope of ABZ_K_LTM around the launches of a gather, whatever the number of values."""
    L = abz._lib
    s = product_series(abz, orc.tb_integer(2))
    dev = s.device()
    rule = dev.rule(8, None, L.WANT_EIG)
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        dev.ctx.prof_reset()
        rule.ltm_green_node_weights(np.linspace(-3, 3, 7) + 0.1j, export=False)
        ms, launches = dev.ctx.prof_read(L.K_LTM)
        assert launches == 1 and ms > 0.0
    finally:
        dev.ctx.prof_enable(False)

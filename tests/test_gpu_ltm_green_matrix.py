"""Band projectors P^b_pq(k) = U_pb conj(U_qb) computed on the device as matrix elements of the tetrahedron method
(abz_rule_ltm_projectors, ltm_proj_lane_kernel / ltm_proj_rows_kernel in kernels_ltm_orb.hip) and the local Green's function
matrix built from them (DeviceRule.ltm_green_matrix, dos.green_local), against LAPACK on the exported H and the numpy
restatement of tests/gloc_ltm_numpy.py.

Shapes: the smallest that reach every kernel path -- 2, 3, 4 bands (one node per lane) on 5^3; 5 bands (NP = 8, 32 nodes per
pass) on a 1-D grid of 40: two passes, the second ragged; 9 bands (NP = 16, 16 nodes per pass) on 17^2: a ragged second pass of
one node; 17 bands (NP = 32) on 5^3 with four selected pairs.

Bounds.  Separated bands (nodes whose smallest gap exceeds 1e-3 of the spectrum's scale): the eigenvector error is
n eps ||H|| / gap <= 17 * 2.2e-16 * 1e3 = 4e-12, the bound on a projector 1e-10.  Completeness and the spectral identity hold at
every node, degenerate or not: 1e-10 max(1, max|H|) on the separated cases, 1e-8 max(1, max|H|) on the degenerate construction,
the project's bound for eigenvector-derived sums.  Green's function: the restatement is fed the exported eigenvalues and the
exported DEVICE projectors, so the bound is the LTM parity bound 1e-9 max(1, max|ref|) on the real and the imaginary part."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import abz_oracle as orc
import gloc_ltm_numpy as gl
import ltm_numpy as ln
from test_gpu_ltm_green import close, product_series, z_lists
from test_gpu_parity import rand_series
from test_ltm_green_matrix_cpu import identity_z, rotated_bands, rotated_reference

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAIRS17 = [(0, 0), (0, 16), (3, 7), (16, 16)]


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def all_pairs(m):
    return [(a, a) for a in range(m)] + [(a, b) for a in range(m) for b in range(a + 1, m)]


def groups_of(pairs):
    """`pairs` dealt in order into groups of at most 16 components (the rule of DeviceRule.ltm_green_matrix)."""
    out, ncomp = [[]], 0
    for p, q in pairs:
        need = 1 if p == q else 2
        if ncomp + need > 16:
            out.append([])
            ncomp = 0
        out[-1].append((p, q))
        ncomp += need
    return out


def device_components(rule, pairs):
    rule.ltm_projectors(pairs)
    A = rule.ltm_elements_export()
    assert A.shape == (gl.ncomponents(pairs), rule.nk, rule.dev.s.n) and np.all(np.isfinite(A)) and rule._ltm_ncomp == len(A)
    return A


def device_tensor(rule, pairs, m, index=None):
    """P [m, m, nk, n] complex of `pairs` from as many attaches as their components need."""
    P = np.zeros((m, m, rule.nk, rule.dev.s.n), dtype=np.complex128)
    for group in groups_of(pairs):
        P += gl.tensor_of_components(device_components(rule, group), group, m, index)
    return P


def make_series(abz, n):
    """(series, npt) of the table above."""
    if n == 5:
        c, first = rand_series(np.random.default_rng(105), (5,), 5, hermitian=True)
        return abz.FourierSeries(c, period=1.0, first=first, ndim=1), 40
    if n == 9:
        c, first = rand_series(np.random.default_rng(209), (3, 5), 9, hermitian=True)
        return abz.FourierSeries(c, period=1.0, first=first, ndim=2), 17
    return product_series(abz, orc.synthetic_wannier(n, rmax=2, seed=7)), 5


def hermitian_upper(H):
    """Hermitian(H): the upper triangle and its conjugate, a real diagonal."""
    up = np.triu(H, 1)
    return up + np.conj(np.swapaxes(up, -1, -2)) + np.real(np.einsum("...ii->...i", H))[..., None] * np.eye(H.shape[-1])


def check_identities(P, pairs, index, e, Hh, bound, what):
    """sum_b P^b_pq = delta_pq and sum_b e_b P^b_pq = H_pq(k) at every node, for the listed pairs."""
    comp = spec = 0.0
    for p, q in pairs:
        i, j = index(p), index(q)
        comp = max(comp, np.abs(P[i, j].sum(axis=-1) - (1.0 if p == q else 0.0)).max())
        spec = max(spec, np.abs((P[i, j] * e).sum(axis=-1) - Hh[:, p, q]).max())
    print(f"projectors {what}: completeness {comp:.3e}, spectral identity {spec:.3e} (bound {bound:.1e})")
    assert comp <= bound and spec <= bound, (what, comp, spec, bound)


# ---------------------------------------------------------------- 1. projectors against LAPACK
@pytest.mark.parametrize("n", [2, 3, 4, 5, 9, 17])
def test_projectors_match_lapack(abz, n):
    L = abz._lib
    s, npt = make_series(abz, n)
    pairs = PAIRS17 if n == 17 else all_pairs(n)
    orbs = sorted({a for pr in pairs for a in pr})
    index = orbs.index
    rule = abz.DeviceRule(s.device(), npt, None, L.WANT_H | L.WANT_EIG)
    try:
        ex = rule.export(x=False, w=False, H=True, eig=True)
        H, e = ex["H"], ex["eig"]
        P = device_tensor(rule, pairs, len(orbs), index)
    finally:
        rule.close()
    scale = max(1.0, np.abs(H).max())
    sep = np.min(np.diff(e, axis=1), axis=1) > 1e-3 * np.abs(e).max()
    assert sep.mean() > 0.9, sep.mean()
    ref = gl.projector_tensor(H[sep])[np.ix_(orbs, orbs)]
    dev = max(np.abs(P[index(p), index(q)][sep] - ref[index(p), index(q)]).max() for p, q in pairs)
    print(f"projectors n={n} npt={npt}: {sep.sum()} of {len(sep)} nodes separated, max dev {dev:.3e} (bound 1e-10)")
    assert dev <= 1e-10
    check_identities(P, pairs, index, e, hermitian_upper(H), 1e-10 * scale, f"n={n} npt={npt}")


def test_projector_of_a_swapped_pair_is_the_conjugate(abz):
    s, npt = make_series(abz, 3)
    rule = abz.DeviceRule(s.device(), npt, None, abz._lib.WANT_EIG)
    a, b = device_components(rule, [(0, 2)]), device_components(rule, [(2, 0)])
    rule.close()
    assert np.array_equal(bits(a[0]), bits(b[0]))  # the real part is symmetric in p and q, product by product
    # the imaginary part changes sign up to the rounding of two products of magnitude <= 1
    assert np.abs(a[1] + b[1]).max() <= 4 * 2.0**-52 and np.abs(a[1]).max() > 1e-2


@pytest.mark.parametrize("n3,mult", [(3, 2), (3, 3)])
def test_projectors_of_degenerate_levels(abz, n3, mult):
    """H = Q (I_mult x h(k)) Q^H of test_orbital_weights_of_degenerate_levels, every level `mult` times: single projectors are
    not defined, the sums over all bands are."""
    L = abz._lib
    rng = np.random.default_rng(7 * n3 + mult)
    c3, first = rand_series(rng, (3, 3, 3), n3, hermitian=True)
    n = n3 * mult
    q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    c = np.einsum("ab,...bc,dc->...ad", q, np.kron(np.eye(mult), c3), q.conj())
    c = 0.5 * (c + np.conj(np.swapaxes(c[::-1, ::-1, ::-1], -1, -2)))  # exactly Hermitian, degenerate to rounding
    s = abz.FourierSeries(c, period=1.0, first=first)
    rule = abz.DeviceRule(s.device(), 5, None, L.WANT_H | L.WANT_EIG)
    ex = rule.export(x=False, w=False, H=True, eig=True)
    pairs = all_pairs(n)
    P = device_tensor(rule, pairs, n)
    rule.close()
    e = ex["eig"]
    assert np.abs(e.reshape(len(e), n3, mult) - e.reshape(len(e), n3, mult)[:, :, :1]).max() <= 1e-9 * np.abs(e).max()
    check_identities(P, pairs, (lambda a: a), e, hermitian_upper(ex["H"]), 1e-8 * max(1.0, np.abs(ex["H"]).max()),
                     f"degenerate {n3} x {mult}")


# ---------------------------------------------------------------- 2. the diagonal pairs are the orbital weights
@pytest.mark.parametrize("n", [3, 9])
def test_diagonal_pairs_equal_the_orbital_weights_to_the_bit(abz, n):
    s, npt = make_series(abz, n)
    rule = abz.DeviceRule(s.device(), npt, None, abz._lib.WANT_EIG)
    rule.ltm_orbitals()
    W = rule.ltm_elements_export()
    D = device_components(rule, [(o, o) for o in range(n)])
    assert np.array_equal(bits(W), bits(D))
    mixed = [(n - 1, n - 1), (0, n - 1), (1, 1)]  # diagonal planes beside an off-diagonal pair
    M = device_components(rule, mixed)
    rule.close()
    assert np.array_equal(bits(M[0]), bits(W[n - 1])) and np.array_equal(bits(M[3]), bits(W[1]))


# ---------------------------------------------------------------- 3. layouts, repeatability
@pytest.mark.parametrize("n", [3, 6, 9, 17])
def test_projectors_do_not_depend_on_the_h_layout(abz, n):
    """3: lane kernel; 6, 9, 17: 8, 16 and 32 lanes per node.  Above 16 bands the library has no compact layout and drops the bit
    (abzhip.h): at n = 17 the third rule is a second full-layout one."""
    L = abz._lib
    s, npt = make_series(abz, n)
    pairs = groups_of(all_pairs(n))[0]
    blocks = []
    for want in (L.WANT_EIG, L.WANT_H | L.WANT_EIG, L.WANT_H | L.WANT_EIG | L.WANT_H_COMPACT):
        rule = abz.DeviceRule(s.device(), npt, None, want)
        A = device_components(rule, pairs)
        assert np.array_equal(bits(A), bits(device_components(rule, pairs))), want  # two calls on one rule
        blocks.append(A)
        rule.close()
    assert np.array_equal(bits(blocks[0]), bits(blocks[1])) and np.array_equal(bits(blocks[0]), bits(blocks[2]))


# ---------------------------------------------------------------- 4. the matrix against the restatement
def matrix_case(abz, name):
    if name == "svo_8":
        return abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz")), 8, 1
    if name == "syn3_5":
        return product_series(abz, orc.synthetic_wannier(3, rmax=2, seed=7)), 5, 1
    c, first = rand_series(np.random.default_rng(305), (3, 3), 5, hermitian=True)  # 5 + 20 components: two groups
    return abz.FourierSeries(c, period=1.0, first=first, ndim=2), 6, 2


def check_matrix(G, ref, what):
    assert G.shape == ref.shape and G.dtype == np.complex128 and np.all(np.isfinite(bits(G))), (what, G.shape, ref.shape)
    dev, bound = close(G, ref)
    print(f"ltm_green_matrix {what}: max dev {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound, (what, dev, bound)


@pytest.mark.parametrize("name", ["syn3_5", "rand5_6", "svo_8"])
def test_green_matrix_matches_restatement(abz, name):
    s, npt, ngroups = matrix_case(abz, name)
    n = s.n
    rule = abz.DeviceRule(s.device(), npt, None, abz._lib.WANT_EIG)
    assert len(groups_of(all_pairs(n))) == ngroups
    eig = ln.rule_eigenvalues(rule)
    P = device_tensor(rule, all_pairs(n), n)
    Pg = P.reshape((n, n) + eig.shape)
    lists = z_lists(eig)
    for label in ("seven", "edges"):
        zs = lists[label]
        G = rule.ltm_green_matrix(zs)
        assert getattr(rule, "_ltm_owner", None) is None
        check_matrix(G, gl.green_matrix(eig, Pg, zs), f"{name} {label}")
        tr = rule.ltm_green(zs)
        dev, bound = close(np.trace(G, axis1=1, axis2=2), tr)
        print(f"ltm_green_matrix {name} {label}: |sum_p G_pp - tr G| {dev:.3e} (bound {bound:.1e})")
        assert dev <= bound
        Gc = rule.ltm_green_matrix(np.conj(zs))
        assert np.array_equal(bits(G.transpose(0, 2, 1)), bits(np.conj(Gc))), (name, label)
        assert np.array_equal(bits(G), bits(rule.ltm_green_matrix(zs)))
    # a selection of orbitals is the sub-block, in the order asked for
    sel = [n - 1, 0]
    Gs = rule.ltm_green_matrix(lists["seven"], orbitals=sel)
    check_matrix(Gs, rule.ltm_green_matrix(lists["seven"])[:, sel][:, :, sel], f"{name} orbitals={sel}")
    rule.close()


# ---------------------------------------------------------------- 5. the exact identity through the device
def test_rotated_bands_through_the_device(abz):
    """H(k) = Q diag(e_b(k)) Q^dagger as a series: c(0) = Q diag(3 b) Q^dagger, c(+-e_j) = Q diag(c_bj / 2) Q^dagger."""
    d, npt, n = 3, 4, 3
    eig, _, q, coef = rotated_bands(d, npt)
    herm = lambda m: 0.5 * (m + m.conj().T)
    c = np.zeros((3,) * d + (n, n), dtype=np.complex128)
    c[1, 1, 1] = herm((q * (3.0 * np.arange(n))) @ q.conj().T)
    for j in range(d):
        m = herm((q * (0.5 * coef[:, j])) @ q.conj().T)
        up, dn = [1] * d, [1] * d
        up[j], dn[j] = 2, 0
        c[tuple(up)] = m
        c[tuple(dn)] = m.conj().T
    s = abz.FourierSeries(c, period=1.0, first=(-1,) * d, ndim=d)
    rule = abz.DeviceRule(s.device(), npt, None, abz._lib.WANT_EIG)
    assert np.abs(np.sort(ln.rule_eigenvalues(rule).reshape(-1, n), axis=0) - np.sort(eig.reshape(-1, n), axis=0)).max() <= 1e-12
    zs = identity_z(eig)
    G = rule.ltm_green_matrix(zs)
    rule.close()
    check_matrix(G, rotated_reference(eig, q, zs), "rotated bands, d = 3")


# ---------------------------------------------------------------- 6. dos.green_local
def test_green_local_on_a_cache(abz):
    h = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    bz = abz.load_bz(abz.FBZ(), 3.85856 * np.eye(3))
    eig0 = ln.rule_eigenvalues(h.device().rule(8, None, abz._lib.WANT_EIG))
    Es = np.linspace(eig0.min() - 0.1, eig0.max() + 0.1, 5)
    zs = Es + 1e-2j
    cache = abz.dos.init(abz.DOSProblem(h, Es, bz), abz.LTM(npt=8))
    G = abz.dos.green_local(cache, zs)
    assert G.shape == (5, 3, 3)
    assert np.array_equal(bits(G), bits(cache.cacheval.ltm_green_matrix(zs)))
    dev, bound = close(np.trace(G, axis1=1, axis2=2), abz.dos.green_trace(cache, zs))
    assert dev <= bound
    assert np.array_equal(bits(abz.dos.green_local(cache, zs, orbitals=[2, 0])), bits(G[:, [2, 0]][:, :, [2, 0]]))
    # mutate in place and set isfresh: H -> H / 2 gives G'(z) = 2 G(2 z)
    h.c[...] = h.c * 0.5
    cache.isfresh = True
    G2 = abz.dos.green_local(cache, 0.5 * zs)
    assert not cache.isfresh
    check_matrix(0.5 * G2, G, "green_local follows the series")
    assert np.abs(abz.dos.green_local(cache, zs) - G).max() > 1e-3
    # a problem instead of a cache
    Gp = abz.dos.green_local(abz.DOSProblem(h, 0.0, bz), zs[:2])
    assert Gp.shape == (2, 3, 3)
    # a cache that attaches device orbital weights finds them gone and attaches them again
    Es2 = 0.5 * Es
    orb = abz.dos.init(abz.DOSProblem(h, Es2, bz), abz.LTM(npt=8, elements="orbitals", eigenvectors="device"))
    u1 = abz.dos.solve_(orb).u
    Go = abz.dos.green_local(orb, 0.5 * zs)
    assert orb.cacheval._ltm_ncomp == 9 and np.array_equal(bits(Go), bits(G2))
    u2 = abz.dos.solve_(orb).u
    assert u2.shape == (5, 3) and np.array_equal(u1, u2)


# ---------------------------------------------------------------- 7. refusals of the C entry point
def test_projectors_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s = product_series(abz, orc.synthetic_wannier(3, rmax=2, seed=7))
    dev = s.device()

    def ptr(pairs):
        a = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        return a, a.ctypes.data_as(L.c_i32p)

    keep, pdiag = ptr([(0, 0), (1, 1), (2, 2)])

    def refused(rc, code, words=None):
        assert rc == code, (rc, code, lib.abz_last_error())
        assert len(lib.abz_last_error()) > 0
        if words is not None:
            assert words in lib.abz_last_error(), lib.abz_last_error()

    def keeps(rule, A, rc, code, words=None):
        refused(rc, code, words)
        assert np.array_equal(rule.ltm_elements_export(), A)

    # rules that are not a whole periodic grid, or hold no eigenvalues
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, 8, cub.syms, L.WANT_EIG)
    refused(lib.abz_rule_ltm_projectors(sym._h, pdiag, 3), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    idx, w = abz.symptr_rule(8, 3, cub.syms)
    irr = C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, 8, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(irr)))
    refused(lib.abz_rule_ltm_projectors(irr, pdiag, 3), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    assert lib.abz_rule_destroy(irr) == 0
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, 8, 2, 6, L.WANT_EIG, C.byref(slab)))
    refused(lib.abz_rule_ltm_projectors(slab, pdiag, 3), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    L.check(lib.abz_rule_ltm_halo(slab))
    refused(lib.abz_rule_ltm_projectors(slab, pdiag, 3), L.ERR_UNSUPPORTED, b"slab")
    assert lib.abz_rule_destroy(slab) == 0
    honly = abz.DeviceRule(dev, 8, None, L.WANT_H)
    refused(lib.abz_rule_ltm_projectors(honly._h, pdiag, 3), L.ERR_ARG)
    honly.close()
    # an unfolded rule takes elements, not projectors
    unf = sym.unfold()
    A = np.random.default_rng(1).standard_normal((2, unf.nk, 3))
    unf.ltm_elements(A)
    keeps(unf, A, lib.abz_rule_ltm_projectors(unf.h, pdiag, 3), L.ERR_UNSUPPORTED, b"unfolded")
    unf.close()
    sym.close()
    # argument checks on a rule that qualifies
    full = abz.DeviceRule(dev, 8, None, L.WANT_EIG)
    A = np.random.default_rng(2).standard_normal((2, full.nk, 3))
    full.ltm_elements(A)
    h = full.h
    keeps(full, A, lib.abz_rule_ltm_projectors(h, None, 3), L.ERR_ARG)
    keeps(full, A, lib.abz_rule_ltm_projectors(h, pdiag, 0), L.ERR_ARG)
    keeps(full, A, lib.abz_rule_ltm_projectors(h, pdiag, -1), L.ERR_ARG)
    for bad in (3, -1, 1 << 20):
        for pair in ((0, bad), (bad, 1)):
            _k, pb = ptr([(0, 1), pair])
            keeps(full, A, lib.abz_rule_ltm_projectors(h, pb, 2), L.ERR_ARG)
    _k9, p9 = ptr([(0, 1)] * 8 + [(2, 2)])  # 17 components in 9 pairs
    keeps(full, A, lib.abz_rule_ltm_projectors(h, p9, 9), L.ERR_ARG, b"components")
    _k17, p17 = ptr([(0, 0)] * 17)
    keeps(full, A, lib.abz_rule_ltm_projectors(h, p17, 17), L.ERR_ARG)
    with pytest.raises(ValueError):
        full.ltm_projectors([(0, 3)])
    with pytest.raises(ValueError):
        full.ltm_projectors([0, 1, 2])
    with pytest.raises(ValueError):
        full.ltm_projectors([(0.5, 1.0)])
    assert np.array_equal(full.ltm_elements_export(), A) and full._ltm_ncomp == 2
    # valid calls afterwards: sixteen components, duplicates are fine
    _k16, p16 = ptr([(0, 1)] * 7 + [(2, 2), (1, 1)])
    assert lib.abz_rule_ltm_projectors(h, p16, 9) == 0
    full._ltm_ncomp = 16
    B = full.ltm_elements_export()
    assert B.shape == (16, full.nk, 3) and np.array_equal(bits(B[0]), bits(B[12])) and np.array_equal(bits(B[1]), bits(B[13]))
    full.ltm_orbitals()
    W = full.ltm_elements_export()
    assert np.array_equal(bits(B[14]), bits(W[2])) and np.array_equal(bits(B[15]), bits(W[1]))
    full.close()
    # above 32 bands there is no kernel
    sn = product_series(abz, orc.synthetic_wannier(33, rmax=2, seed=7))
    rule = abz.DeviceRule(sn.device(), 5, None, L.WANT_EIG)
    A = np.ones((1, rule.nk, 33))
    rule.ltm_elements(A)
    keeps(rule, A, lib.abz_rule_ltm_projectors(rule.h, pdiag, 3), L.ERR_UNSUPPORTED, b"33 bands")
    rule.close()
    # a series that is not Hermitian
    c, first = rand_series(np.random.default_rng(9), (3, 3, 3), 3, hermitian=False)
    rule = abz.DeviceRule(abz.FourierSeries(c, period=1.0, first=first).device(), 5, None, L.WANT_H | L.WANT_EIG)
    A = np.ones((1, rule.nk, 3))
    rule.ltm_elements(A)
    keeps(rule, A, lib.abz_rule_ltm_projectors(rule.h, pdiag, 3), L.ERR_ARG, b"Hermitian")
    rule.close()


def test_projectors_are_accounted(abz):
    """abz_mem_info: refusals and transient rules leave nothing behind, and the bytes and blocks return to their value when the
    rule goes."""
    L = abz._lib
    s, npt = make_series(abz, 9)
    dev = s.device()
    info = lambda: (dev.ctx.mem_info()[0], dev.ctx.mem_info()[4])
    bad = np.array([[0, 9]], dtype=np.int32)

    def cycle():
        m0 = info()
        rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
        m1 = info()
        assert L.lib().abz_rule_ltm_projectors(rule.h, bad.ctypes.data_as(L.c_i32p), 1) == L.ERR_ARG
        assert info() == m1
        rule.ltm_projectors([(0, 8), (3, 3)])
        m2 = info()
        rule.ltm_projectors([(1, 2)])  # replaces the block
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
    print(f"mem (bytes, blocks): before {m0}, rule {m1}, three components {m2}, two components {m3}, destroyed {m4}")
    assert m2[1] == m1[1] + 1 and m3[1] == m1[1] + 1 and m4 == m0


# ---------------------------------------------------------------- 8. refusals of the Python mirrors
def test_python_refusals(abz):
    L = abz._lib
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    zs = np.array([0.5 + 1e-2j])
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.dos.init(abz.DOSProblem(s, 0.0, cub), abz.LTM(npt=8, symmetric=True))
    with pytest.raises(ValueError, match="symmetric"):
        abz.dos.green_local(sym, zs)
    with pytest.raises(ValueError):
        abz.dos.green_local(abz.dos.init(abz.DOSProblem(s, 0.0, cub), abz.GGR(npt=8)), zs)
    full = abz.DeviceRule(dev, 8, None, L.WANT_EIG)
    with pytest.raises(ValueError, match="real"):
        full.ltm_green_matrix([0.5])
    with pytest.raises(ValueError):
        full.ltm_green_matrix(zs, orbitals=[])
    with pytest.raises(ValueError, match="twice"):
        full.ltm_green_matrix(zs, orbitals=[0, 0])
    full.close()
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        rule = dev.rule(8, None, L.WANT_EIG)
        with pytest.raises(NotImplementedError, match="halo"):
            rule.ltm_projectors([(0, 0)])
        with pytest.raises(NotImplementedError, match="halo"):
            rule.ltm_green_matrix(zs)
        rule.ltm_halo()
        with pytest.raises(NotImplementedError, match="ltm_projectors"):
            rule.ltm_projectors([(0, 0)])
        with pytest.raises(NotImplementedError, match="ltm_green_matrix"):
            rule.ltm_green_matrix(zs)
        with pytest.raises(NotImplementedError, match="green_local"):
            abz.dos.green_local(abz.DOSProblem(s, 0.0, bz), zs)
    finally:
        dev.kshard, dev.allreduce = None, None

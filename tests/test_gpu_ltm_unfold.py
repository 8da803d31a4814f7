"""Tetrahedron DOS from irreducible nodes on the device (abz_rule_ltm_unfold; ltm_rank_kernel, ltm_orbit_kernel and
ltm_unfold_kernel of kernels_ltm.hip): the gather against the numpy orbit map of tests/unfold_numpy.py, the scans of the
unfolded rule against the restatements of tests/ltm_numpy.py / tests/wltm_numpy.py and against the full-grid rule of the
same series, the reference's DOS test with LTM(symmetric=True), the Fermi level, the cache, refusals and bookkeeping.

Symmetry sets: InversionSymIBZ is the group of the 2^d sign flips and CubicSymIBZ adds the axis permutations
(src/brillouin.jl:248-307).  The integer models, SVO and the symmetrised synthetic series have both.  Graphene in its
oblique lattice basis has none of the single-axis mirrors (its eigenvalues move by 1.6 under k_1 -> -k_1) and is run under
the inversion proper, {1, -1}: the symmetries handed to an unfold must be symmetries of H.

Parity bound everywhere: |u - ref| <= 1e-9 max(1, max|ref|), the project's (test_gpu_ltm.py).
"""
import ctypes as C
import gc
import os
import re

import numpy as np
import pytest

import abz_oracle as orc
import ltm_numpy as ln
import unfold_numpy as un
import wltm_numpy as wn
from test_gpu_ltm import check_parity, close, energy_lists, product_series
from test_gpu_ltm import make_case as plain_case
from test_gpu_ltm_weighted import check, on_grid
from test_ltm_cpu import MODELS, reference_energies
from test_ltm_unfold_cpu import model_sym_sets

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CASES = [("int1", "inversion"), ("int1", "cubic"), ("int2", "inversion"), ("int2", "cubic"), ("graphene", "inversion"),
         ("int3", "inversion"), ("int3", "cubic"), ("svo", "inversion"), ("svo", "cubic"), ("syn6", "inversion"), ("syn6", "cubic"),
         ("syn16", "inversion"), ("syn16", "cubic"), ("syn17", "inversion"), ("syn17", "cubic"), ("syn33", "inversion"), ("syn33", "cubic")]


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def make_case(abz, name):
    """(series, npt): int1 101, int2 40, graphene 36, int3 24, SVO 20^3, cubic-symmetrised synthetic series at 12^3."""
    if name.startswith("syn"):
        return product_series(abz, un.symmetrise(orc.synthetic_wannier(int(name[3:]), rmax=2, seed=7))), 12
    return plain_case(abz, name)


def rules(abz, name, label):
    """(source rule on the irreducible nodes, its unfolded rule, the full-grid rule of the same series, syms)"""
    L = abz._lib
    s, npt = make_case(abz, name)
    dev = s.device()
    syms = model_sym_sets(abz, name, s.d)[label]
    src = abz.DeviceRule(dev, npt, syms, L.WANT_EIG)
    return src, src.unfold(), dev.rule(npt, None, L.WANT_EIG), syms


def int_syms(syms, d):
    return np.ascontiguousarray(np.rint(np.asarray(syms)).astype(np.int32).reshape(-1, d, d))


def c_unfold(L, src_h, S, out, nsyms=None, null_syms=False):
    return L.lib().abz_rule_ltm_unfold(src_h, None if null_syms else S.ctypes.data_as(L.c_i32p), len(S) if nsyms is None else nsyms,
                                       C.byref(out) if out is not None else None)


def check_copy(src, unf, full, syms):
    d, npt = src.dev.s.d, src.npt
    se = src.export(eig=True)
    ue = unf.export(eig=True)
    node_of = un.orbit_map(npt, d, syms, se["x"])
    assert unf.nk == npt ** d == len(ue["eig"]) and unf.npt == npt
    assert np.array_equal(np.bincount(node_of, minlength=src.nk), se["w"].astype(np.int64))
    assert np.array_equal(ue["eig"], se["eig"][node_of])
    fe = full.export()
    assert np.array_equal(ue["x"], fe["x"]) and np.array_equal(ue["w"], fe["w"]) and np.all(ue["w"] == 1.0)
    return node_of


# ---------------------------------------------------------------- 1. the gather is a copy
@pytest.mark.parametrize("name,label", CASES)
def test_unfold_is_a_copy(abz, name, label):
    src, unf, full, syms = rules(abz, name, label)
    assert isinstance(unf, abz.UnfoldedRule) and src.unfold() is unf
    check_copy(src, unf, full, syms)
    print(f"unfold {name} {label}: {src.nk} of {unf.nk} nodes")


def test_unfold_of_an_explicit_node_list(abz, monkeypatch):
    """A source built from symptr_rule's list on the host (abz_ptr_rule_build with irr_idx), and one from a list that keeps
    ANOTHER representative of every orbit than the smallest image."""
    L = abz._lib
    monkeypatch.setenv("ABZ_SYM_DEVICE", "0")
    src, unf, full, syms = rules(abz, "svo", "cubic")
    check_copy(src, unf, full, syms)
    dev, npt = src.dev, src.npt
    idx, w = abz.symptr_rule(npt, 3, syms)
    other = un.grid_points(npt, 3)[un.images(npt, 3, syms)[-1][un.flat_index(idx, npt)]].astype(np.int32)
    assert not np.array_equal(other, idx)
    other = np.ascontiguousarray(other)
    h = C.c_void_p()
    L.check(L.lib().abz_ptr_rule_build(dev.h, npt, len(w), other.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(h)))
    out = C.c_void_p()
    S = int_syms(syms, 3)
    try:
        L.check(c_unfold(L, h, S, out))
        n = dev.s.n
        got, src_eig = np.empty((npt ** 3, n)), np.empty((len(w), n))
        L.check(L.lib().abz_rule_export(out, None, None, None, got.ctypes.data_as(L.c_f64p), None))
        L.check(L.lib().abz_rule_export(h, None, None, None, src_eig.ctypes.data_as(L.c_f64p), None))
        node_of = un.orbit_map(npt, 3, syms, other / npt)
        assert np.array_equal(got, src_eig[node_of])
        dev_, bound = close(got, unf.export(eig=True)["eig"])
        print(f"explicit list of other representatives against the device-built list: eigenvalues differ by {dev_:.3e}")
        assert dev_ <= bound
    finally:
        L.lib().abz_rule_destroy(out)
        L.lib().abz_rule_destroy(h)


# ---------------------------------------------------------------- 2. parity with the restatement
@pytest.mark.parametrize("name,label", CASES)
def test_unfolded_ltm_matches_restatement(abz, name, label):
    src, unf, full, syms = rules(abz, name, label)
    eig = ln.rule_eigenvalues(unf)
    assert np.all(np.diff(eig, axis=-1) >= 0.0)
    worst = 0.0
    for what, Es in energy_lists(eig, np.random.default_rng(5)).items():
        worst = max(worst, check_parity(unf, Es, eig, what=f"unfolded {name} {label} npt={unf.npt} {what}"))
    print(f"unfolded ltm parity {name} {label}: worst deviation / bound = {worst:.3e}")


@pytest.mark.parametrize("name,label", [("int3", "cubic"), ("svo", "cubic")])
def test_unfolded_weighted_ltm_matches_restatement(abz, name, label):
    src, unf, full, syms = rules(abz, name, label)
    eig = ln.rule_eigenvalues(unf)
    n = eig.shape[-1]
    A = np.random.default_rng(17).standard_normal((3, unf.nk, n))
    lists = energy_lists(eig, np.random.default_rng(5))
    unf.ltm_elements(A)
    for what, Es in lists.items():
        ref_e = wn.wltm(eig, eig, Es)
        ref_a = wn.wltm(eig, on_grid(unf, A), Es)
        for states in (False, True):
            tag = f"unfolded {name} {what} {'N' if states else 'g'}"
            check(unf.ltm(Es, states=states, elements="energy"), ref_e[1 if states else 0], tag + " energy")
            check(unf.ltm(Es, states=states, elements="attached"), ref_a[1 if states else 0], tag + " ncomp=3")
    unf.ltm_elements(None)


# ---------------------------------------------------------------- 3. against the full-grid rule of the same series
@pytest.mark.parametrize("name,label", CASES)
def test_unfolded_against_the_full_grid_rule(abz, name, label):
    """Eigenvalues and the g / N sums on the linspace300 and many1500 lists.  The `edges` list is left out on purpose: it
    holds exact corner eigenvalues, where g is discontinuous in one dimension and an ulp decides the region."""
    src, unf, full, syms = rules(abz, name, label)
    eu, ef = ln.rule_eigenvalues(unf), ln.rule_eigenvalues(full)
    de, be = close(eu, ef)
    print(f"unfolded vs full {name} {label}: eigenvalues differ by {de:.3e} (bound {be:.1e})")
    assert de <= be
    lists = energy_lists(ef, np.random.default_rng(5))
    for what in ("linspace300", "many1500"):
        Es = lists[what]
        for states in (False, True):
            ref = full.ltm(Es, states=states)
            dev, bound = close(unf.ltm(Es, states=states), ref)
            print(f"unfolded vs full {name} {label} {what} {'N' if states else 'g'}: max dev {dev:.3e} (bound {bound:.1e}, max|ref| {np.abs(ref).max():.3g})")
            assert dev <= bound, (name, label, what, states, dev, bound)


# ---------------------------------------------------------------- 4. the reference's DOS test with the new switch
@pytest.mark.parametrize("name", ["int1", "int2", "graphene", "int3"])
def test_symmetric_ltm_vs_exact_dos(abz, name):
    """ref: test/dos.jl:88-111 with LTM(npt=200, symmetric=True): |u - exact| < 1e-2 at the reference's ten energies, and within
    the parity bound of the symmetric=False value."""
    make, exact, B = MODELS[name]
    so = make()
    Es = reference_energies(B)
    if name == "graphene":
        bz = abz.load_bz(abz.FBZ(), np.eye(2))
        bz.syms = model_sym_sets(abz, name, 2)["inversion"]
        zones = {"inversion {1, -1}": bz}
    else:
        zones = {type(k).__name__: abz.load_bz(k, np.eye(so.d)) for k in (abz.InversionSymIBZ(), abz.CubicSymIBZ())}

    def sweep(bz, symmetric):
        s = product_series(abz, so)
        cache = abz.dos.init(abz.DOSProblem(s, 0.0, bz), abz.LTM(npt=200, symmetric=symmetric))
        assert isinstance(cache.cacheval, abz.UnfoldedRule) == symmetric
        us = []
        for e in Es:
            cache.domain = e
            sol = abz.dos.solve_(cache)
            assert isinstance(sol.u, float) and sol.retcode
            us.append(sol.u)
        return np.array(us)

    for kind, bz in zones.items():
        u = sweep(bz, True)
        err = max(abs(a - exact(e)) for a, e in zip(u, Es))
        plain = sweep(bz, False)
        dev, bound = close(u, plain)
        print(f"symmetric ltm vs exact {name} {kind}: max err {err:.3e}; against symmetric=False {dev:.3e} (bound {bound:.1e})")
        assert err < 1e-2, (name, kind, u)
        assert dev <= bound, (name, kind, dev, bound)


def test_symmetric_ltm_on_the_full_zone_is_the_plain_rule(abz):
    s = product_series(abz, orc.tb_integer(2))
    cache = abz.dos.init(abz.DOSProblem(s, 0.5, abz.load_bz(abz.FBZ(), np.eye(2))), abz.LTM(npt=16, symmetric=True))
    assert not isinstance(cache.cacheval, abz.UnfoldedRule) and cache.cacheval.syms is None
    plain = abz.dos.solve(abz.DOSProblem(product_series(abz, orc.tb_integer(2)), 0.5, abz.load_bz(abz.FBZ(), np.eye(2))), abz.LTM(npt=16)).u
    assert abz.dos.solve_(cache).u == plain


def test_symmetric_ltm_elements(abz):
    """elements="energy" and a callable on a symmetric cache: evaluated at every full-grid node of the unfolded rule."""
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    bz = abz.load_bz(abz.CubicSymIBZ(), 3.85856 * np.eye(3))
    Es = np.linspace(11.5, 14.5, 33)
    f = lambda x, eig: np.stack([eig, np.cos(2 * np.pi * x[:, :1]) ** 2 + 0 * eig])
    for elements in ("energy", f):
        cache = abz.dos.init(abz.DOSProblem(s, Es, bz), abz.LTM(npt=12, elements=elements, symmetric=True))
        rule = cache.cacheval
        assert isinstance(rule, abz.UnfoldedRule)
        u = abz.dos.solve_(cache).u
        eig = ln.rule_eigenvalues(rule)
        ex = rule.export(x=True, w=False, eig=True)
        A = eig if elements == "energy" else on_grid(rule, f(ex["x"], ex["eig"]))
        check(u, wn.wltm(eig, A, Es)[0], f"symmetric cache, elements {'energy' if elements == 'energy' else 'callable'}")
    with pytest.raises(ValueError, match="orbitals"):
        abz.dos.init(abz.DOSProblem(s, Es, bz), abz.LTM(npt=12, elements="orbitals", symmetric=True))


# ---------------------------------------------------------------- 5. Fermi level
def test_unfolded_fermi_level_svo(abz):
    """A metallic filling, nstates = 1 of 3 bands, tol 1e-9: both searches end in an interval no wider than tol, and
    eigenvalues that differ in the last digits can move the crossing by one interval, so |dE_F| <= 2 tol; and the bracket
    property of abz_rule_ltm_fermi's contract on the unfolded rule itself (test_gpu_ltm_weighted.py::test_fermi_level_svo)."""
    src, unf, full, syms = rules(abz, "svo", "cubic")
    nstates, tol = 1.0, 1e-9
    ef, nf = unf.ltm_fermi(nstates, tol)
    ef_full, _ = full.ltm_fermi(nstates, tol)
    N = unf.ltm(np.array([ef, ef - 2 * tol]), states=True)
    print(f"fermi unfolded svo: E_F = {ef:.12f}, full grid {ef_full:.12f} (apart {abs(ef - ef_full):.3e}), N(E_F) - nstates = {N[0] - nstates:.3e}, "
          f"N(E_F - 2 tol) - nstates = {N[1] - nstates:.3e}")
    assert abs(ef - ef_full) <= 2 * tol
    assert N[0] >= nstates * (1 - 1e-12)
    assert N[1] < nstates
    assert abs(nf - N[0]) <= 1e-9 * 3
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    cache = abz.dos.init(abz.DOSProblem(s, 0.0, abz.load_bz(abz.CubicSymIBZ(), 3.85856 * np.eye(3))), abz.LTM(npt=20, symmetric=True))
    assert isinstance(cache.cacheval, abz.UnfoldedRule)
    ef2, _ = abz.dos.fermi_level(cache, nstates, tol)
    assert abs(ef2 - ef) <= tol


# ---------------------------------------------------------------- 6. the cache follows the series
def test_symmetric_ltm_cache_follows_the_series(abz):
    """The shape of test_ltm_cache_follows_the_series with symmetric=True: the 1-D cosine band on the inversion-reduced zone."""
    L = abz._lib
    make = lambda scale: abz.FourierSeries(scale * np.array([0.5, 0.0, 0.5]).reshape(3, 1, 1), period=1.0, offset=-2)
    h = make(1.0)
    bz = abz.load_bz(abz.InversionSymIBZ(), [[2 * np.pi]])
    E = 0.3
    alg = abz.LTM(symmetric=True)
    cache = abz.dos.init(abz.DOSProblem(h, E, bz), alg)
    rule = cache.cacheval
    assert isinstance(rule, abz.UnfoldedRule) and rule.source.nk == 26 and rule.nk == 50
    k = np.arange(50) / 50.0

    def expect(scale):
        eig = ln.rule_eigenvalues(cache.cacheval)
        assert np.abs(eig - (scale * np.cos(2 * np.pi * k))[:, None]).max() <= 1e-12 * scale
        return ln.ltm(eig, [E])[0][0]

    fresh = lambda scale: abz.dos.solve(abz.DOSProblem(make(scale), E, bz), alg).u
    sol1 = abz.dos.solve_(cache)
    r1 = expect(1.0)
    assert r1 > 0 and abs(sol1.u - r1) <= 1e-9 * max(1.0, r1) and sol1.u == fresh(1.0)
    h.c *= 2
    cache.isfresh = True
    sol2 = abz.dos.solve_(cache)
    r2 = expect(2.0)
    assert cache.cacheval is rule and not cache.isfresh  # the same handle, gathered again through its orbit map
    assert abs(sol2.u - r2) <= 1e-9 * max(1.0, r2) and sol2.u == fresh(2.0) and abs(sol2.u - sol1.u) > 1e-3
    cache.H = make(4.0)
    assert cache.isfresh
    sol3 = abz.dos.solve_(cache)
    r3 = expect(4.0)
    assert abs(sol3.u - r3) <= 1e-9 * max(1.0, r3) and sol3.u == fresh(4.0) and abs(sol3.u - sol2.u) > 1e-3
    # attached elements are dropped by a refresh
    rule = cache.cacheval
    rule.ltm_elements(np.ones((2, rule.nk, 1)))
    Es = np.array([E])
    assert rule.ltm(Es, elements="attached").shape == (1, 2)
    rule.rebuild()
    out = np.full(2, -99.0)
    rc = L.lib().abz_rule_ltm_weighted(rule.h, L.LTM_A_ELEMENTS, Es.ctypes.data_as(L.c_f64p), 1, L.LTM_DOS, out.ctypes.data_as(L.c_f64p))
    assert rc == L.ERR_ARG and len(L.lib().abz_last_error()) > 0 and np.all(out == -99.0)
    with pytest.raises(ValueError):
        rule.ltm(Es, elements="attached")
    rule.ltm_elements(np.ones((2, rule.nk, 1)))
    cache.H.c *= 0.5
    cache.isfresh = True
    sol4 = abz.dos.solve_(cache)
    assert sol4.u == fresh(2.0)
    with pytest.raises(ValueError):
        cache.cacheval.ltm(Es, elements="attached")


# ---------------------------------------------------------------- 7. refusals and bookkeeping
def test_unfold_refusals(abz):
    L = abz._lib
    lib = L.lib()
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    S = int_syms(cub.syms, 3)
    npt = 8

    def refused(rc, code, match=None):
        msg = lib.abz_last_error().decode()
        assert rc == code and len(msg) > 0, (rc, code, msg)
        if match:
            assert re.search(match, msg), msg
        return msg

    sym = abz.DeviceRule(dev, npt, cub.syms, L.WANT_EIG)
    honly = abz.DeviceRule(dev, npt, cub.syms, L.WANT_H)
    full = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    out = C.c_void_p()
    refused(c_unfold(L, honly._h, S, out), L.ERR_ARG, "eigenvalues")
    refused(c_unfold(L, full._h, S, out), L.ERR_UNSUPPORTED, "nothing to unfold")
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, npt, 2, 6, L.WANT_EIG, C.byref(slab)))
    refused(c_unfold(L, slab, S, out), L.ERR_UNSUPPORTED, "nothing to unfold")
    refused(c_unfold(L, sym._h, S, out, nsyms=0), L.ERR_ARG)
    refused(c_unfold(L, sym._h, S, out, nsyms=-3), L.ERR_ARG)
    refused(c_unfold(L, sym._h, S, out, null_syms=True), L.ERR_ARG)
    refused(c_unfold(L, sym._h, S, None), L.ERR_ARG)
    refused(c_unfold(L, None, S, out), L.ERR_ARG)
    assert not out.value
    # *out that is not an unfolded rule of the same npt, d, n, series
    L.check(c_unfold(L, sym._h, S, out))
    good = out.value
    L.check(c_unfold(L, sym._h, S, out))  # a refresh keeps the handle
    assert out.value == good
    notunf = C.c_void_p(full._h.value)
    refused(c_unfold(L, sym._h, S, notunf), L.ERR_ARG, "not a rule made by")
    srcself = C.c_void_p(sym._h.value)
    refused(c_unfold(L, sym._h, S, srcself), L.ERR_ARG)
    sym9 = abz.DeviceRule(dev, 9, cub.syms, L.WANT_EIG)
    refused(c_unfold(L, sym9._h, S, out), L.ERR_ARG, "another geometry")
    s2 = product_series(abz, orc.tb_integer(3))
    sym_other = abz.DeviceRule(s2.device(), npt, cub.syms, L.WANT_EIG)
    refused(c_unfold(L, sym_other._h, S, out), L.ERR_ARG, "another geometry")
    inv = abz.load_bz(abz.InversionSymIBZ(), np.eye(3))
    sym_inv = abz.DeviceRule(dev, npt, inv.syms, L.WANT_EIG)  # same series and npt, another node count
    refused(c_unfold(L, sym_inv._h, int_syms(inv.syms, 3), out), L.ERR_ARG, "another geometry")
    refused(c_unfold(L, sym._h, np.ascontiguousarray(S[::-1]), out), L.ERR_ARG, "another symmetry set")  # the same group in another order
    refused(c_unfold(L, sym._h, S, out, nsyms=len(S) - 1), L.ERR_ARG, "another symmetry set")
    assert out.value == good
    # an unfolded rule is itself nothing to unfold, and has no plan to rebuild from
    again = C.c_void_p()
    refused(c_unfold(L, out, S, again), L.ERR_UNSUPPORTED, "nothing to unfold")
    refused(lib.abz_rule_rebuild(out), L.ERR_UNSUPPORTED, "abz_rule_ltm_unfold")
    # after the refusals the rule still scans
    Es = np.array([0.5, 1.5])
    res = np.zeros(2)
    assert lib.abz_rule_ltm(out, Es.ctypes.data_as(L.c_f64p), 2, L.LTM_DOS, res.ctypes.data_as(L.c_f64p)) == 0
    dev_, bound = close(res, ln.ltm(ln.rule_eigenvalues(full), Es)[0])
    assert dev_ <= bound
    # the symmetries of a smaller group than the list was made for leave orbits uncovered; so does a list with a node removed
    idx, w = abz.symptr_rule(npt, 3, cub.syms)
    short = C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, npt, len(w) - 1, idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(short)))
    m0 = dev.ctx.mem_info()[0]
    msg = refused(c_unfold(L, short, S, again), L.ERR_ARG, r"do(es)? not cover every orbit")
    assert int(re.search(r"unfold: (\d+) of the", msg).group(1)) == int(w[-1]) and not again.value
    assert dev.ctx.mem_info()[0] == m0  # the half-made rule, its map and the scratch are gone
    msg = refused(c_unfold(L, sym._h, int_syms(inv.syms, 3), again), L.ERR_ARG, "not cover every orbit")
    assert int(re.search(r"unfold: (\d+) of the", msg).group(1)) > 0 and not again.value
    assert lib.abz_rule_destroy(short) == 0 and lib.abz_rule_destroy(slab) == 0 and lib.abz_rule_destroy(out) == 0
    # the Python mirror
    with pytest.raises(ValueError, match="full grid"):
        full.unfold()
    with pytest.raises(ValueError, match="eigenvalues"):
        honly.unfold()
    u = sym.unfold()
    with pytest.raises(ValueError, match="full grid"):
        u.unfold()
    dev.kshard, dev.allreduce = (0, 2), (lambda a: a)
    try:
        with pytest.raises(NotImplementedError):
            dev.rule(npt, cub.syms, L.WANT_EIG).unfold()
    finally:
        dev.kshard, dev.allreduce = None, None


def test_unfold_memory_is_accounted(abz):
    L = abz._lib
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    dev = s.device()
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    npt, n = 24, 3

    def cycle(source_first):
        m0 = dev.ctx.mem_info()[0]
        src = abz.DeviceRule(dev, npt, cub.syms, L.WANT_EIG)
        m1 = dev.ctx.mem_info()[0]
        unf = src.unfold()
        m2 = dev.ctx.mem_info()[0]
        unf.rebuild()  # a refresh allocates nothing that stays
        m2b = dev.ctx.mem_info()[0]
        first, second = (src, unf) if source_first else (unf, src)
        first.close()
        Es = np.linspace(11.0, 14.0, 16)
        if source_first:
            assert np.all(np.isfinite(unf.ltm(Es)))  # the unfolded rule does not hold its source
        second.close()
        m3 = dev.ctx.mem_info()[0]
        return m0, m1, m2, m2b, m3

    gc.collect()
    gc.disable()
    try:
        cycle(True)  # the context's scratch buffers and the cached symmetric-rule tables grow once
        for source_first in (True, False):
            m0, m1, m2, m2b, m3 = cycle(source_first)
            print(f"mem: start {m0}, source {m1}, unfolded {m2} (+{m2 - m1}: planes {8 * n * npt ** 3} + map {4 * npt ** 3}), closed {m3}")
            assert m2 - m1 >= (8 * n + 4) * npt ** 3
            assert m2b == m2 and m3 == m0
    finally:
        gc.enable()


def test_unfold_launches_are_profiled_and_repeatable(abz):
    """The map (rank + orbit kernels) and the gather are one ProfScope of ABZ_K_LTM each: 2 at the first call, 1 per refresh.
    Two unfolds of the same source give bit-identical planes."""
    L = abz._lib
    s = abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    dev = s.device()
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    src = abz.DeviceRule(dev, 16, cub.syms, L.WANT_EIG)
    S = int_syms(cub.syms, 3)
    a, b = C.c_void_p(), C.c_void_p()
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        dev.ctx.prof_reset()
        L.check(c_unfold(L, src.h, S, a))
        ms, launches = dev.ctx.prof_read(L.K_LTM)
        assert launches == 2 and ms > 0.0
        L.check(c_unfold(L, src.h, S, a))
        assert dev.ctx.prof_read(L.K_LTM)[1] == 3
        assert dev.ctx.prof_read(L.K_GGR)[1] == 0
    finally:
        dev.ctx.prof_enable(False)
    try:
        L.check(c_unfold(L, src.h, S, b))
        ea, eb = np.empty((16 ** 3, 3)), np.empty((16 ** 3, 3))
        L.check(L.lib().abz_rule_export(a, None, None, None, ea.ctypes.data_as(L.c_f64p), None))
        L.check(L.lib().abz_rule_export(b, None, None, None, eb.ctypes.data_as(L.c_f64p), None))
        assert np.array_equal(ea, eb)
        nk, n, d, npt, want = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        L.check(L.lib().abz_rule_info(a, C.byref(nk), C.byref(n), C.byref(d), C.byref(npt), C.byref(want)))
        assert (nk.value, n.value, d.value, npt.value, want.value) == (16 ** 3, 3, 3, 16, L.WANT_EIG)
    finally:
        L.lib().abz_rule_destroy(a)
        L.lib().abz_rule_destroy(b)

"""The allocator's books (abz_mem_info: live bytes, live blocks) around the entry points that allocate: a repeated call
leaves them where they were, a refusal leaves them where they were, and handles destroyed in any order give everything
back.  Tiny shapes only: 2 (and 6) bands, 3 x 3 coefficients, grids of 6 to 8 points, straight on the C ABI."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NPT = 8
# the inversion / mirror symmetries of the square
SYMS = np.ascontiguousarray(np.array([[[1, 0], [0, 1]], [[-1, 0], [0, -1]], [[1, 0], [0, -1]], [[-1, 0], [0, 1]]], dtype=np.int32))


@pytest.fixture(scope="module")
def L():
    import autobzcore.jl_amd as m
    return m._lib


def coefficients(n, seed, hermitian=True):
    """[3][3][n][n] complex coefficients of a 2-D series in the ABI's order, as float64 pairs."""
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((3, 3, n, n)) + 1j * rng.standard_normal((3, 3, n, n))) / np.sqrt(n)
    if hermitian:  # c(-R) = c(R)^dagger, exactly
        c = 0.5 * (c + np.conj(np.swapaxes(c[::-1, ::-1], -1, -2)))
    return np.ascontiguousarray(np.ascontiguousarray(c).view(np.float64).reshape(-1))


def create_ctx(L):
    h = C.c_void_p()
    L.check(L.lib().abz_ctx_create(0, C.byref(h)))
    return h


def create_series(L, ctx, n, seed=1):
    h = C.c_void_p()
    dims, first, per = np.array([3, 3], dtype=np.int32), np.array([-1, -1], dtype=np.int32), np.ones(2)
    L.check(L.lib().abz_series_create(ctx, coefficients(n, seed).ctypes.data_as(L.c_f64p), 2, dims.ctypes.data_as(L.c_i32p),
                                      first.ctypes.data_as(L.c_i32p), per.ctypes.data_as(L.c_f64p), n, C.byref(h)))
    return h


@pytest.fixture(scope="module")
def world(L):
    """One context and the 2-band and 6-band series every case below shares (and, under tuple keys, rules that cases keep)."""
    ctx = create_ctx(L)
    w = {"ctx": ctx, 2: create_series(L, ctx, 2), 6: create_series(L, ctx, 6)}
    yield w
    destroy(L, *[r for key, r in w.items() if isinstance(key, tuple)])
    for n in (2, 6):
        assert L.lib().abz_series_destroy(w[n]) == 0
    assert L.lib().abz_ctx_destroy(ctx) == 0


def books(L, ctx):
    info = (C.c_int64 * 5)()
    L.check(L.lib().abz_mem_info(ctx, info))
    return int(info[0]), int(info[4])  # live bytes, live blocks


def sym_nodes(L, ctx, syms=SYMS, npt=NPT):
    nirr = C.c_int64(0)
    ps = syms.ctypes.data_as(L.c_i32p)
    L.check(L.lib().abz_symptr_rule_device(ctx, npt, 2, ps, len(syms), C.byref(nirr), None, None))
    idx, w = np.zeros((nirr.value, 2), dtype=np.int32), np.zeros(nirr.value, dtype=np.int64)
    L.check(L.lib().abz_symptr_rule_device(ctx, npt, 2, ps, len(syms), C.byref(nirr), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p)))
    return idx, w


def build_list(L, s, idx, w, want, npt=NPT):
    r = C.c_void_p()
    rc = L.lib().abz_ptr_rule_build(s, npt, len(w), idx.ctypes.data_as(L.c_i32p) if len(w) else None,
                                    w.ctypes.data_as(L.c_i64p) if len(w) else None, want, C.byref(r))
    return rc, r


def build_full(L, s, want, npt=NPT):
    rc, r = build_list(L, s, np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=np.int64), want, npt)
    L.check(rc)
    return r


def build_sym(L, s, want, syms=SYMS, npt=NPT):
    r = C.c_void_p()
    L.check(L.lib().abz_ptr_rule_build_sym(s, npt, syms.ctypes.data_as(L.c_i32p), len(syms), want, C.byref(r)))
    return r


def unfold(L, src, syms, out):
    return L.lib().abz_rule_ltm_unfold(src, syms.ctypes.data_as(L.c_i32p), len(syms), C.byref(out))


def destroy(L, *rules):
    for r in rules:
        assert L.lib().abz_rule_destroy(r) == 0


def kept(w, key, make):
    """The rule that the cases share under `key`, made at its first use (the world's teardown destroys it)."""
    if key not in w:
        w[key] = make()
    return w[key]


def attach_elements(L, r, n, ncomp=2, npt=NPT):
    A = np.random.default_rng(3).standard_normal((ncomp, npt * npt, n))
    L.check(L.lib().abz_rule_ltm_elements(r, A.ctypes.data_as(L.c_f64p), ncomp))


# ---------------------------------------------------------------- steady state
def call_eval_nodes(L, w, n):
    k = np.random.default_rng(5).random((100, 2))
    H, E = np.zeros((100, n * n, 2)), np.zeros((100, n))
    L.check(L.lib().abz_eval_nodes(w[n], k.ctypes.data_as(L.c_f64p), 100, L.WANT_H | L.WANT_EIG, H.ctypes.data_as(L.c_f64p),
                                   E.ctypes.data_as(L.c_f64p)))
    assert np.all(np.isfinite(H)) and np.all(np.isfinite(E))


def call_ptr_sum(L, w, n):
    eta, om, out = np.array([0.3]), np.array([0.1, 0.4]), np.zeros((2, 2))
    L.check(L.lib().abz_ptr_sum(w[n], NPT, 0, NPT, L.F_DOS, eta.ctypes.data_as(L.c_f64p), 1, om.ctypes.data_as(L.c_f64p), 2, 1,
                                out.ctypes.data_as(L.c_f64p)))
    assert np.all(np.isfinite(out))


def call_sym_rule(L, w, n):
    sym_nodes(L, w["ctx"])
    destroy(L, build_sym(L, w[n], L.WANT_H | L.WANT_EIG))


def call_list_rule(L, w, n):
    idx, wt = sym_nodes(L, w["ctx"])
    rc, r = build_list(L, w[n], idx, wt, L.WANT_H | L.WANT_EIG)
    L.check(rc)
    destroy(L, r)


def call_ltm_elements(L, w, n):
    r = kept(w, ("full_eig", n), lambda: build_full(L, w[n], L.WANT_EIG))
    attach_elements(L, r, n)
    L.check(L.lib().abz_rule_ltm_elements(r, None, 0))


def call_ltm_orbitals(L, w, n):
    r = kept(w, ("full_eig", n), lambda: build_full(L, w[n], L.WANT_EIG))  # eigenvalues only: H(k) comes from a transient rule
    L.check(L.lib().abz_rule_ltm_orbitals(r, None, 0))
    L.check(L.lib().abz_rule_ltm_elements(r, None, 0))


def call_unfold(L, w, n):
    src = kept(w, ("sym_eig", n), lambda: build_sym(L, w[n], L.WANT_EIG))
    out = C.c_void_p()
    L.check(unfold(L, src, SYMS, out))
    destroy(L, out)


def call_halo(L, w, n):
    slab = C.c_void_p()
    L.check(L.lib().abz_ptr_rule_build_slab(w[n], NPT, 2, 5, L.WANT_EIG, C.byref(slab)))
    L.check(L.lib().abz_rule_ltm_halo(slab))
    destroy(L, slab)


def call_contract_grow(L, w, n):
    """A level pool grown past its first size keeps its earlier slots (a copy into a bigger block); on a series of its own, so
    that every run grows one."""
    s = create_series(L, w["ctx"], n, seed=9)
    rng = np.random.default_rng(11)
    for count, first_slot in ((2, 0), (40, 2)):
        par, x, slots = np.zeros(count, dtype=np.int64), rng.random(count), np.zeros(count, dtype=np.int64)
        L.check(L.lib().abz_contract_nodes(s, 2, par.ctypes.data_as(L.c_i64p), x.ctypes.data_as(L.c_f64p), count, slots.ctypes.data_as(L.c_i64p)))
        assert slots[0] == first_slot and slots[-1] == first_slot + count - 1
    L.check(L.lib().abz_release_level(s, 2))
    assert L.lib().abz_series_destroy(s) == 0


def call_autoptr(L, w, n):
    eta, out, err = np.array([0.5]), np.zeros(2), np.zeros(1)
    nev, npt_out = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32)
    L.check(L.lib().abz_autoptr_solve(w[n], None, 0, L.F_DOS, eta.ctypes.data_as(L.c_f64p), 1, 0.2, 6, 1, 1e-3, 0.0, 400, 0, 1.0,
                                      out.ctypes.data_as(L.c_f64p), err.ctypes.data_as(L.c_f64p), nev.ctypes.data_as(L.c_i64p),
                                      npt_out.ctypes.data_as(L.c_i32p)))
    assert np.all(np.isfinite(out)) and 7 <= npt_out[0] <= 11  # (400 evaluations are reached with the grid of 11 points)
    L.check(L.lib().abz_series_drop_rules(w[n]))


STEADY = [(f, n) for f in (call_eval_nodes, call_ptr_sum, call_sym_rule, call_list_rule) for n in (2, 6)] + \
         [(f, 2) for f in (call_ltm_elements, call_ltm_orbitals, call_unfold, call_halo, call_contract_grow, call_autoptr)] + \
         [(call_ltm_orbitals, 6), (call_autoptr, 6)]


@pytest.mark.parametrize("call,n", STEADY, ids=[f"{f.__name__[5:]}-{n}" for f, n in STEADY])
def test_books_are_steady(L, world, call, n):
    """The first run warms the scratch of the context and the series; the second and the third leave the same books."""
    call(L, world, n)
    b1 = books(L, world["ctx"])
    call(L, world, n)
    b2 = books(L, world["ctx"])
    call(L, world, n)
    b3 = books(L, world["ctx"])
    print(f"(live bytes, live blocks) after runs 1, 2, 3: {b1}, {b2}, {b3}")
    assert b2 == b3


# ---------------------------------------------------------------- refusals after allocation
def refused(L, rc, code, match):
    msg = L.lib().abz_last_error().decode()
    assert rc == code and re.search(match, msg), (rc, code, msg)


def test_refusal_node_outside_the_grid(L, world):
    ctx, s = world["ctx"], world[2]
    idx, wt = sym_nodes(L, ctx)
    bad = idx.copy()
    bad[len(wt) // 2, 1] = NPT
    b0 = books(L, ctx)
    rc, r = build_list(L, s, bad, wt, L.WANT_H)
    refused(L, rc, L.ERR_ARG, rf"irr_idx\[{2 * (len(wt) // 2) + 1}\] = {NPT} outside the grid")
    assert not r.value and books(L, ctx) == b0
    rc, r = build_list(L, s, idx, wt, L.WANT_H)
    assert rc == 0
    destroy(L, r)


def test_refusal_unfold_of_a_list_that_misses_an_orbit(L, world):
    ctx, s = world["ctx"], world[2]
    idx, wt = sym_nodes(L, ctx)
    rc, short = build_list(L, s, idx[:-1], wt[:-1], L.WANT_EIG)
    L.check(rc)
    out = C.c_void_p()
    b0 = books(L, ctx)
    refused(L, unfold(L, short, SYMS, out), L.ERR_ARG, rf"unfold: {int(wt[-1])} of the {NPT * NPT} grid points have no image .* not cover every orbit")
    assert not out.value and books(L, ctx) == b0  # the half-made rule, its map and the scratch are gone
    rc, whole = build_list(L, s, idx, wt, L.WANT_EIG)
    L.check(rc)
    L.check(unfold(L, whole, SYMS, out))
    destroy(L, out, whole, short)


def test_refusal_unfold_into_a_rule_of_another_symmetry_set(L, world):
    ctx, s = world["ctx"], world[2]
    src = build_sym(L, s, L.WANT_EIG)
    out = C.c_void_p()
    L.check(unfold(L, src, SYMS, out))
    kept = out.value
    attach_elements(L, out, 2)
    b0 = books(L, ctx)
    refused(L, unfold(L, src, np.ascontiguousarray(SYMS[::-1]), out), L.ERR_ARG, "another symmetry set")
    assert out.value == kept and books(L, ctx) == b0  # (refused before the attached elements would have been dropped)
    ncomp = C.c_int(0)
    L.check(L.lib().abz_rule_ltm_elements_export(out, C.byref(ncomp), None))
    assert ncomp.value == 2
    L.check(unfold(L, src, SYMS, out))  # the refresh it was made for still works (and drops the elements)
    assert out.value == kept
    destroy(L, out, src)


def test_refusal_rebuild_of_a_compact_rule_of_a_series_no_longer_hermitian(L, world):
    ctx = world["ctx"]
    s = create_series(L, ctx, 2, seed=4)
    r = build_full(L, s, L.WANT_H | L.WANT_H_COMPACT | L.WANT_EIG)
    want = C.c_int(0)
    L.check(L.lib().abz_rule_info(r, None, None, None, None, C.byref(want)))
    assert want.value & L.WANT_H_COMPACT
    L.check(L.lib().abz_series_update(s, coefficients(2, 4, hermitian=False).ctypes.data_as(L.c_f64p)))
    b0 = books(L, ctx)
    refused(L, L.lib().abz_rule_rebuild(r), L.ERR_ARG, "keeps H\\(k\\) as an upper triangle .* no longer Hermitian: build a new rule")
    assert books(L, ctx) == b0
    L.check(L.lib().abz_series_update(s, coefficients(2, 4).ctypes.data_as(L.c_f64p)))
    L.check(L.lib().abz_rule_rebuild(r))
    assert books(L, ctx) == b0
    destroy(L, r)
    assert L.lib().abz_series_destroy(s) == 0


# ---------------------------------------------------------------- destroy in any order
@pytest.mark.parametrize("order", ["ctx-rule-series", "series-rule-ctx"])
def test_destroy_in_any_order(L, world, order):
    b0 = books(L, world["ctx"])
    ctx = create_ctx(L)
    s = create_series(L, ctx, 2, seed=6)
    rule = build_sym(L, s, L.WANT_EIG)
    child = C.c_void_p()
    L.check(unfold(L, rule, SYMS, child))
    attach_elements(L, child, 2)
    full = build_full(L, s, L.WANT_H | L.WANT_EIG)
    attach_elements(L, full, 2)
    assert books(L, ctx)[1] > b0[1]
    for what in order.split("-"):
        if what == "ctx":
            assert L.lib().abz_ctx_destroy(ctx) == 0
        elif what == "series":
            assert L.lib().abz_series_destroy(s) == 0
        else:
            destroy(L, child, rule, full)
    fresh = create_ctx(L)
    assert books(L, fresh) == b0
    assert L.lib().abz_ctx_destroy(fresh) == 0

"""LTM on slabs of the grid (abz_rule_ltm_halo; the slab instantiations of ltm_window_kernel, both payloads, in
kernels_ltm.hip; DeviceRule.ltm_halo and dos.solve(..., LTM()) under dist.kshard) against the slab restatement of
tests/slab_ltm_numpy.py and against the whole-grid scans.

One GPU plays every rank in turn: `dev.kshard, dev.allreduce = (r, W), (lambda a: a)`, the ranks' results are summed here.
The restatement is fed the whole-grid rule's own exported eigenvalues, so only summation order and FMA contraction remain
(and, where the slab's builder differs from the whole grid's, the last digits of its eigenvalues); the bound is the
project's parity bound |u - ref| <= 1e-9 max(1, max|ref|) (test_gpu_ltm.py), twice that between two device results."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import abz_oracle as orc
import bloechl_numpy as bn
import ltm_numpy as ln
import slab_ltm_numpy as sn
from test_gpu_ltm import GOLD, close, energy_lists, product_series

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


@contextlib.contextmanager
def as_rank(dev, r, W):
    """This GPU as rank r of W: the shard is set, the all-reduce is the identity (the test sums the ranks itself)."""
    saved = (dev.kshard, dev.allreduce)
    dev.kshard, dev.allreduce = (r, W), (lambda a: a)
    try:
        yield
    finally:
        dev.kshard, dev.allreduce = saved


def make_series(abz, name):
    if name == "int3":
        return product_series(abz, orc.tb_integer(3))
    if name == "int2":
        return product_series(abz, orc.tb_integer(2))
    if name == "graphene":
        return product_series(abz, orc.tb_graphene())
    if name == "svo":
        return abz.load_w90_series(os.path.join(GOLD, "svo_hr.dat.gz"))
    return product_series(abz, orc.synthetic_wannier(int(name[3:]), rmax=2, seed=7))


def slab_rules(abz, dev, npt, W, want):
    """[(z0, z1, rule with its halo)] of the W ranks, built one after another on this GPU (not through the series' cache)."""
    out = []
    for r, (z0, z1) in enumerate(sn.slabs(npt, W)):
        with as_rank(dev, r, W):
            rule = abz.DeviceRule(dev, npt, None, want)
            rule.ltm_halo()
        out.append((z0, z1, rule))
    return out


def scan(dev, rule, Es, **kw):
    with as_rank(dev, *rule.shard):
        return rule.ltm(Es, **kw)


def wants(abz, name):
    L = abz._lib
    if name != "svo":
        return {"eig": L.WANT_EIG}
    # eigenvalue planes alone, behind 2 n^2 matrix planes, behind n^2 (upper triangle): three tile strides, and the halo's own
    return {"eig": L.WANT_EIG, "H+eig": L.WANT_H | L.WANT_EIG, "compact": L.WANT_H | L.WANT_EIG | L.WANT_H_COMPACT}


# ---------------------------------------------------------------- 1. parity per slab, and the slabs add up
PARITY = [("int3", 5, 5), ("int3", 12, 5), ("graphene", 13, 3), ("int2", 7, 7), ("svo", 8, 3), ("syn16", 6, 2), ("syn33", 6, 2)]


@pytest.mark.parametrize("name,npt,W", PARITY, ids=[f"{n}-{p}x{w}" for n, p, w in PARITY])
def test_slab_ltm_matches_restatement_and_adds_up(abz, name, npt, W):
    L = abz._lib
    s = make_series(abz, name)
    dev = s.device()
    full = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    eig = ln.rule_eigenvalues(full)
    n = eig.shape[-1]
    lists = energy_lists(eig, np.random.default_rng(5))
    whole = {(label, st): full.ltm(Es, states=st) for label, Es in lists.items() for st in (False, True)}
    refs = {}  # the restatement of every slab, once for all layouts
    for z0, z1 in sn.slabs(npt, W):
        ext = sn.extend(eig, z0, z1)
        for label, Es in lists.items():
            refs[(z0, label)] = sn.ltm(ext, Es)
    worst, worst_sum = 0.0, 0.0
    for wlabel, want in wants(abz, name).items():
        rules = slab_rules(abz, dev, npt, W, want)
        if wlabel == "compact":
            assert all(r.want & L.WANT_H_COMPACT for _, _, r in rules)
        # below the bands of the reference AND of the slabs' own planes (another builder may differ in the last digit)
        lo = min([eig.min()] + [r.export(x=False, w=False, eig=True)["eig"].min() for _, _, r in rules])
        for label, Es in lists.items():
            below = Es < lo
            assert below.any() or label == "one"
            for st in (False, True):
                total, ref_total = np.zeros(len(Es)), np.zeros(len(Es))
                for z0, z1, rule in rules:
                    u = scan(dev, rule, Es, states=st)
                    ref = refs[(z0, label)][1 if st else 0]
                    assert u.shape == ref.shape and np.all(np.isfinite(u))
                    dv, bound = close(u, ref)
                    assert dv <= bound, (name, wlabel, label, st, (z0, z1), dv, bound)
                    worst = max(worst, dv)
                    assert np.all(u[below] == 0.0)  # exactly 0 below the bands on every slab (g and N)
                    total += u
                    ref_total += ref
                w = whole[(label, st)]
                dv = np.abs(total - w).max()
                bound = 2e-9 * max(1.0, np.abs(ref_total).max())
                assert dv <= bound, (name, wlabel, label, st, dv, bound)
                worst_sum = max(worst_sum, dv)
                if st and label == "linspace300":  # its last energy lies above all bands
                    assert Es[-1] > eig.max() and abs(total[-1] - n) <= 1e-12 * n, total[-1]
        z0, z1, rule = rules[-1]
        for st in (False, True):  # the same bits at every call
            Es = lists["many1500"]
            assert np.array_equal(scan(dev, rule, Es, states=st), scan(dev, rule, Es, states=st))
        for _, _, rule in rules:
            rule.close()
    print(f"slab ltm {name} npt={npt} W={W}: largest deviation slab vs restatement {worst:.3e}, sum of slabs vs whole grid {worst_sum:.3e}")


# ---------------------------------------------------------------- 2. energy-weighted sums
WEIGHTED = [("int3", 12, 5), ("graphene", 13, 3), ("svo", 8, 3)]


@pytest.mark.parametrize("name,npt,W", WEIGHTED, ids=[f"{n}-{p}x{w}" for n, p, w in WEIGHTED])
def test_slab_energy_weighted_sums(abz, name, npt, W):
    """g_A, N_A and the corrected N_A with A = e (ABZ_LTM_A_ENERGY), the checks and bounds of the plain scans."""
    L = abz._lib
    s = make_series(abz, name)
    dev = s.device()
    full = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    eig = ln.rule_eigenvalues(full)
    lists = energy_lists(eig, np.random.default_rng(5))
    modes = {"g_A": dict(states=False), "N_A": dict(states=True), "N_A corrected": dict(states=True, correction=True)}
    rules = slab_rules(abz, dev, npt, W, L.WANT_EIG)
    worst, worst_sum = 0.0, 0.0
    lo = min([eig.min()] + [r.export(x=False, w=False, eig=True)["eig"].min() for _, _, r in rules])
    for label, Es in lists.items():
        below = Es < lo
        refs = []
        for z0, z1, _ in rules:
            ext = sn.extend(eig, z0, z1)
            sx = sn.sorted_simplices(ext, ext)
            g, N = sn.wltm_from(sx, Es)
            refs.append({"g_A": g, "N_A": N, "N_A corrected": N + bn.correction_from(sx, Es)})
        for mode, kw in modes.items():
            total, ref_total = np.zeros((len(Es), 1)), np.zeros((len(Es), 1))
            for (z0, z1, rule), ref in zip(rules, refs):
                u = scan(dev, rule, Es, elements="energy", **kw)
                assert u.shape == (len(Es), 1) and np.all(np.isfinite(u))
                dv, bound = close(u, ref[mode])
                assert dv <= bound, (name, label, mode, (z0, z1), dv, bound)
                worst = max(worst, dv)
                assert np.all(u[below] == 0.0)
                total += u
                ref_total += ref[mode]
            w = full.ltm(Es, elements="energy", **kw)
            dv = np.abs(total - w).max()
            bound = 2e-9 * max(1.0, np.abs(ref_total).max())
            assert dv <= bound, (name, label, mode, dv, bound)
            worst_sum = max(worst_sum, dv)
    rule = rules[0][2]
    for kw in modes.values():
        Es = lists["seven"]
        assert np.array_equal(scan(dev, rule, Es, elements="energy", **kw), scan(dev, rule, Es, elements="energy", **kw))
    print(f"slab energy-weighted {name} npt={npt} W={W}: largest deviation slab vs restatement {worst:.3e}, "
          f"sum of slabs vs whole grid {worst_sum:.3e}")


# ---------------------------------------------------------------- 3. the halo follows the series
def test_halo_follows_the_series(abz):
    """5^3 in 5 slabs of one plane: every cell reads the halo, a stale one would be wrong everywhere.  New coefficients in
    place + invalidate(): the slab's refill (abz_rule_rebuild) refills the halo; a second abz_rule_ltm_halo does too."""
    L = abz._lib
    s = make_series(abz, "int3")
    dev = s.device()
    npt, W = 5, 5
    full = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    rules = slab_rules(abz, dev, npt, W, L.WANT_EIG)
    eig0 = ln.rule_eigenvalues(full)
    Es = np.linspace(eig0.min() - 0.1, eig0.max() + 0.1, 41)
    before = [scan(dev, rule, Es, states=True) for _, _, rule in rules]
    s.c[0, 1, 1] *= 1.75  # the hoppings along the first and the last axis, by different factors: every plane, and so
    s.c[2, 1, 1] *= 1.75  # the halo, changes whichever of them the outermost variable is
    s.c[1, 1, 0] *= 0.6
    s.c[1, 1, 2] *= 0.6
    s.invalidate()
    eig = ln.rule_eigenvalues(full)  # (refilled by its handle)
    assert np.abs(eig - eig0).max() > 0.1
    Es = np.linspace(eig.min() - 0.1, eig.max() + 0.1, 41)
    worst = 0.0
    for again in (False, True):
        for (z0, z1, rule), old in zip(rules, before):
            if again and rule._h is not None:
                L.check(L.lib().abz_rule_ltm_halo(rule._h))
            ext = sn.extend(eig, z0, z1)
            for st in (False, True):
                u = scan(dev, rule, Es, states=st)
                ref = sn.ltm(ext, Es)[1 if st else 0]
                dv, bound = close(u, ref)
                assert dv <= bound, (again, (z0, z1), st, dv, bound)
                worst = max(worst, dv)
            assert np.abs(scan(dev, rule, Es, states=True) - old).max() > 1e-3
    print(f"halo follows the series: largest deviation {worst:.3e}")


# ---------------------------------------------------------------- 4. the Python path
def test_dos_solve_under_kshard(abz):
    so = orc.tb_integer(3)
    bz = abz.load_bz(abz.FBZ(), np.eye(3))
    Es = np.linspace(-6.5, 6.5, 53)
    algs = {"g": dict(), "N": dict(cumulative=True), "corrected band energy": dict(cumulative=True, elements="energy", correction=True)}
    worst = 0.0
    for npt, W in ((12, 5), (5, 7)):  # W = 7 at npt = 5: two ranks hold no plane and give zeros
        for label, kw in algs.items():
            s = product_series(abz, so)
            dev = s.device()
            ref = np.asarray(abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=npt, **kw)).u)
            total = np.zeros_like(ref)
            empty = 0
            for r in range(W):
                with as_rank(dev, r, W):
                    sol = abz.dos.solve(abz.DOSProblem(s, Es, bz), abz.LTM(npt=npt, **kw))
                u = np.asarray(sol.u)
                assert sol.retcode and u.shape == ref.shape
                if sn.slabs(npt, W)[r][0] == sn.slabs(npt, W)[r][1]:
                    assert np.all(u == 0.0)
                    empty += 1
                total += u
            assert empty == (2 if W == 7 else 0)
            dv = np.abs(total - ref).max()
            bound = 2e-9 * max(1.0, np.abs(ref).max())
            print(f"dos.solve under kshard npt={npt} W={W} {label}: sum of ranks vs unsharded {dv:.3e} (bound {bound:.1e})")
            assert dv <= bound, (npt, W, label, dv, bound)
            worst = max(worst, dv)
    print(f"dos.solve under kshard: largest deviation {worst:.3e}")


def test_python_refusals_under_kshard(abz):
    L = abz._lib
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    fbz = abz.load_bz(abz.FBZ(), np.eye(3))
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    Es = np.array([0.5, 1.5])
    with as_rank(dev, 0, 2):
        for alg in (abz.LTM(npt=8, elements="orbitals"), abz.LTM(npt=8, elements="orbitals", eigenvectors="device"),
                    abz.LTM(npt=8, elements=lambda x, e: np.ones((1,) + e.shape))):
            with pytest.raises(NotImplementedError, match="k-sharded"):
                abz.dos.init(abz.DOSProblem(s, Es, fbz), alg)
        with pytest.raises(NotImplementedError, match="symmetric"):
            abz.dos.init(abz.DOSProblem(s, Es, cub), abz.LTM(npt=8, symmetric=True))
        with pytest.raises(NotImplementedError, match="all-reduce"):
            abz.dos.fermi_level(abz.DOSProblem(s, Es, fbz), 0.5)
        cache = abz.dos.init(abz.DOSProblem(s, Es, fbz), abz.LTM(npt=8))
        with pytest.raises(NotImplementedError, match="all-reduce"):
            abz.dos.band_energy(cache, 0.5)
        rule = cache.cacheval  # a slab with its halo: everything but the two scans names the limit
        assert rule._ltm_halo and rule.nbytes == 8 * (4 * 64 + 64)
        for call in (lambda: rule.ltm(Es, elements="attached"), lambda: rule.ltm(Es, elements=np.ones((1, 512, 1))),
                     lambda: rule.ltm_fermi(0.5), lambda: rule.ltm_elements(np.ones((1, 512, 1))), lambda: rule.ltm_orbitals(),
                     rule.ltm_elements_export, rule.unfold):
            with pytest.raises(NotImplementedError, match="slab"):
                call()
        assert np.all(np.isfinite(rule.ltm(Es)))  # and the scans still run
        with pytest.raises(NotImplementedError):
            dev.rule(8, cub.syms, L.WANT_EIG).ltm_halo()
    with pytest.raises(ValueError, match="not k-sharded"):
        dev.rule(8, None, L.WANT_EIG).ltm_halo()
    # the symmetric switch on a zone without symmetries is the plain grid, sharded or not
    with as_rank(dev, 1, 2):
        assert abz.dos.init(abz.DOSProblem(s, Es, fbz), abz.LTM(npt=8, symmetric=True)).cacheval._ltm_halo


# ---------------------------------------------------------------- 5. refusals and accounting of the C ABI
def test_halo_refusals_and_accounting(abz):
    L = abz._lib
    lib = L.lib()
    s = product_series(abz, orc.tb_integer(3))
    dev = s.device()
    npt = 8
    Es = np.array([0.5, 1.5])
    out = np.full(2, -99.0)
    pE, pout = Es.ctypes.data_as(L.c_f64p), out.ctypes.data_as(L.c_f64p)

    def refused(rc, code, words=None):
        assert rc == code, (rc, code, lib.abz_last_error())
        assert len(lib.abz_last_error()) > 0
        if words:
            assert words in lib.abz_last_error(), lib.abz_last_error()
        assert np.all(out == -99.0)  # nothing was launched or written

    def slab_of(z0, z1, want):
        h = C.c_void_p()
        L.check(lib.abz_ptr_rule_build_slab(dev.h, npt, z0, z1, want, C.byref(h)))
        return h

    full = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    eig = ln.rule_eigenvalues(full)
    # the refusal table
    refused(lib.abz_rule_ltm_halo(full._h), L.ERR_ARG, b"nothing to attach")
    honly = slab_of(2, 6, L.WANT_H)
    refused(lib.abz_rule_ltm_halo(honly), L.ERR_ARG, b"eigenvalues")
    refused(lib.abz_rule_ltm(honly, pE, 2, L.LTM_DOS, pout), L.ERR_ARG)
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    sym = abz.DeviceRule(dev, npt, cub.syms, L.WANT_EIG)
    refused(lib.abz_rule_ltm_halo(sym._h), L.ERR_UNSUPPORTED, b"irreducible nodes")
    idx, w = abz.symptr_rule(npt, 3, cub.syms)
    irr = C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, npt, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(irr)))
    refused(lib.abz_rule_ltm_halo(irr), L.ERR_UNSUPPORTED, b"irreducible nodes")
    unf = sym.unfold()
    refused(lib.abz_rule_ltm_halo(unf._h), L.ERR_UNSUPPORTED, b"unfolded")
    for h in (sym._h, irr):  # left as they were: still no grid to the scan
        refused(lib.abz_rule_ltm(h, pE, 2, L.LTM_DOS, pout), L.ERR_UNSUPPORTED, b"not a whole periodic grid")
    assert lib.abz_rule_ltm(unf._h, pE, 2, L.LTM_DOS, pout) == 0  # ... and the unfolded grid still one
    dv, bound = close(out, ln.ltm(ln.rule_eigenvalues(unf), Es)[0])
    assert dv <= bound
    out[:] = -99.0
    # a slab without its halo is refused as before, and told how to get one
    slab = slab_of(2, 6, L.WANT_EIG)
    refused(lib.abz_rule_ltm(slab, pE, 2, L.LTM_DOS, pout), L.ERR_UNSUPPORTED, b"attach it with abz_rule_ltm_halo")
    assert b"not a whole periodic grid (a slab of the outermost variable)" in lib.abz_last_error()
    refused(lib.abz_rule_ltm_weighted(slab, L.LTM_A_ENERGY, pE, 2, L.LTM_STATES, pout), L.ERR_UNSUPPORTED, b"attach it with abz_rule_ltm_halo")
    assert lib.abz_rule_ltm_halo(slab) == 0
    m2 = dev.ctx.mem_info()[0]
    # with the halo: everything but the two scans still refuses the slab, and names the limit
    A = np.ones((1, 4 * npt * npt, 1))
    nc = C.c_int(-5)
    orb = np.zeros(1, dtype=np.int32)
    ef = C.c_double(0.0)
    box = C.c_void_p()
    S = np.ascontiguousarray(np.rint(np.asarray(cub.syms)).astype(np.int32).reshape(-1, 3, 3))
    for rc in (lib.abz_rule_ltm_elements(slab, A.ctypes.data_as(L.c_f64p), 1),
               lib.abz_rule_ltm_orbitals(slab, orb.ctypes.data_as(L.c_i32p), 1),
               lib.abz_rule_ltm_elements_export(slab, C.byref(nc), None),
               lib.abz_rule_ltm_fermi(slab, 0.5, 1e-8, C.byref(ef), None),
               lib.abz_rule_ltm_weighted(slab, L.LTM_A_ELEMENTS, pE, 2, L.LTM_DOS, pout)):
        refused(rc, L.ERR_UNSUPPORTED, b"not a whole periodic grid")
        assert b"slab" in lib.abz_last_error()
    refused(lib.abz_rule_ltm_unfold(slab, S.ctypes.data_as(L.c_i32p), len(S), C.byref(box)), L.ERR_UNSUPPORTED, b"slab")
    assert not box.value
    refused(lib.abz_rule_ltm(slab, pE, 2, L.LTM_STATES_CORRECTED, pout), L.ERR_ARG)
    refused(lib.abz_rule_ltm(slab, pE, 0, L.LTM_DOS, pout), L.ERR_ARG)
    assert dev.ctx.mem_info()[0] == m2
    # a valid call afterwards works
    assert lib.abz_rule_ltm(slab, pE, 2, L.LTM_DOS, pout) == 0
    dv, bound = close(out, sn.ltm(sn.extend(eig, 2, 6), Es)[0])
    print(f"after the refusals: slab [2, 6) of 8^3 deviates {dv:.3e} (bound {bound:.1e})")
    assert dv <= bound
    # the launch counts of a slab call are those of the whole-grid call with the same energies
    many = np.linspace(eig.min(), eig.max(), 1500)
    res = np.zeros(1500)
    pm, pres = many.ctypes.data_as(L.c_f64p), res.ctypes.data_as(L.c_f64p)
    dev.ctx.prof_enable(True, kernels=[L.K_LTM])
    try:
        counts = {}
        for label, h in (("slab", slab), ("whole", full._h)):
            for nE in (2, 1500):
                for what in (L.LTM_DOS, L.LTM_STATES):
                    dev.ctx.prof_reset()
                    assert lib.abz_rule_ltm(h, pm, nE, what, pres) == 0
                    counts[(label, nE, what, "plain")] = dev.ctx.prof_read(L.K_LTM)[1]
                for what in (L.LTM_DOS, L.LTM_STATES, L.LTM_STATES_CORRECTED):
                    dev.ctx.prof_reset()
                    assert lib.abz_rule_ltm_weighted(h, L.LTM_A_ENERGY, pm, nE, what, pres) == 0
                    counts[(label, nE, what, "energy")] = dev.ctx.prof_read(L.K_LTM)[1]
        for (label, nE, what, kind), c in counts.items():
            if label == "slab":
                assert c == counts[("whole", nE, what, kind)] >= 1, (nE, what, kind, c)
    finally:
        dev.ctx.prof_enable(False)
    assert lib.abz_rule_destroy(slab) == 0
    assert lib.abz_rule_destroy(honly) == 0 and lib.abz_rule_destroy(irr) == 0
    # the halo is the rule's (the context's scratch has its size by now): its bytes are counted, a second call refills the same
    # blocks, and everything goes with the rule
    m0 = dev.ctx.mem_info()[0]
    slab = slab_of(2, 6, L.WANT_EIG)
    m1 = dev.ctx.mem_info()[0]
    assert lib.abz_rule_ltm_halo(slab) == 0
    m2 = dev.ctx.mem_info()[0]
    plane = 8 * npt * 16  # npt lines of one plane, rows padded to 16 doubles
    assert m2 - m1 >= plane, (m1, m2)
    assert lib.abz_rule_ltm_halo(slab) == 0
    assert lib.abz_rule_ltm(slab, pE, 2, L.LTM_STATES, pout) == 0
    assert dev.ctx.mem_info()[0] == m2
    assert lib.abz_rule_destroy(slab) == 0
    assert dev.ctx.mem_info()[0] == m0

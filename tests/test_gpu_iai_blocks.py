"""The IAI building-block entry points (abz_contract_nodes, abz_eval_line_nodes, abz_release_level) through their Python
mirror on DeviceSeries, against the numpy restatement of tests/iai_blocks_numpy.py.

Only these entry points reach: slots appended behind live ones (with the pool growing under them), the node-list dispatch
of launch_node_integrand (panels15 = false), an arbitrary parent per node, and the host-side argument checks.

Which band count covers which dispatch family of launch_node_integrand (section a, every d in 1..3):
  n = 1, 2, 3, 4     node_integrand_kernel<N, FID> on unpacked level-1 sets (n = 1 also F_LINEAR / F_LINEAR_X)
  n = 5, 8, 9, 16    launch_gen_nodes without the panel kernel: gen_node_kernel (wave per node)
  n = 17, 32         the same for tr G / DOS of Hermitian series, F_ONE and F_DOS_EIG; G, and everything of a series that
                     is not Hermitian: the big_inverse_wanted route into launch_big_nodes
  n = 33, 64         launch_big_nodes: traces of Hermitian series from the tridiagonal form, the rest from the inverse

Bars (section a) are the project's own for the same quantities (tests/test_gpu_fuzz.py): 1e-12 of max|ref| for n <= 4
(F_DOS_EIG: 1e-11, the digit fuzz_small_band_rules grants the eigenvalue form), 1e-10 for n >= 5.  The restatement chain
itself is within 7e-15 of abz_oracle.evaluate_direct on these shapes.

Measured on an MI355X, worst deviation / bar per family over all of section a (every test prints its own):
  node_integrand_kernel, n <= 4        4.8e-01   (4.8e-13 of max|ref|: d = 2, n = 3, not Hermitian; 0.15 and less elsewhere)
  gen_node_kernel, 5..16 bands         8.1e-03
  gen_node_kernel, 17..32 bands        5.2e-05
  big inverse, 17..32 bands            1.9e-02
  big inverse, 33..64 bands            7.0e-03
  big tridiagonal, 33..64 bands        9.0e-06
Sections b-d hold to the bit (np.array_equal) in every family; section c: 4.7e-15 / 1.6e-14 of max|ref| on the slots made
before the pool grew, 2.6e-15 / 5.3e-15 on the last ones; section e: 1155, 16155 and 2835 evaluations, equal to the
oracle's and to abz_iai_solve's, values within 2e-16 of both.
"""
import ctypes as C

import numpy as np
import pytest

import abz_oracle as orc
import iai_blocks_numpy as ib
from test_gpu_fuzz import _herm_series
from test_iai_blocks_cpu import DRIVER_CASES, driver_case

pytestmark = pytest.mark.gpu

PERIOD = (1.0, 2.0, 0.5)
SWEPT = (ib.F_DOS, ib.F_TRGLOC, ib.F_GLOC, ib.F_DOS_EIG)
NAMES = {ib.F_ONE: "one", ib.F_LINEAR: "linear", ib.F_LINEAR_X: "linear_x", ib.F_DOS: "dos", ib.F_TRGLOC: "trgloc",
         ib.F_GLOC: "gloc", ib.F_DOS_EIG: "dos_eig"}


@pytest.fixture(scope="module")
def abz():
    import autobzcore.jl_amd as m
    return m


def make_series(abz, rng, d, n, herm, dims=None):
    """(product series, oracle series).  Not Hermitian: an even M, non-centred first frequencies and, for d = 3, an M = 1
    (the middle variable; for d = 2 it would make every level-1 set the same and the parents of a node meaningless);
    Hermitian (H_{-R} = H_R^dagger needs centred odd axes): the same with M = 3.  Scaled by 1 / sqrt(n)."""
    if herm:
        dims = {1: (3,), 2: (3, 3), 3: (3, 1, 3)}[d] if dims is None else dims
        c, first = _herm_series(rng, dims, n, 1.0 / np.sqrt(n))
    else:
        m1 = 4 if n < 17 else 3
        dims = {1: (m1,), 2: (m1, 3), 3: (m1, 1, 3)}[d] if dims is None else dims
        c = (rng.standard_normal(dims + (n, n)) + 1j * rng.standard_normal(dims + (n, n))) / np.sqrt(n)
        first = (-2, 0, -4)[:d]
    assert len(dims) == d
    s = abz.FourierSeries(c, period=PERIOD[:d], first=first, ndim=d)
    so = orc.FourierSeries(c, period=PERIOD[:d], first=first, ndim=d)
    assert s.device().hermitian() == herm
    return s, so


def accepted(n):
    """Integrand ids abz_eval_line_nodes takes for n bands, and the status of the ones it refuses."""
    L_ARG, L_UNSUP = -1, -4
    if n == 1:
        return list(range(7)), {}
    if n <= 32:
        return [ib.F_ONE, ib.F_DOS, ib.F_TRGLOC, ib.F_GLOC, ib.F_DOS_EIG], {ib.F_LINEAR: L_ARG, ib.F_LINEAR_X: L_ARG}
    return [ib.F_DOS, ib.F_TRGLOC, ib.F_GLOC], {ib.F_LINEAR: L_ARG, ib.F_LINEAR_X: L_ARG, ib.F_ONE: L_UNSUP, ib.F_DOS_EIG: L_UNSUP}


def family(n, herm, fid):
    if n <= 4:
        return "node_integrand_kernel n<=4"
    inverse = fid in (ib.F_DOS, ib.F_TRGLOC, ib.F_GLOC) and (not herm or fid == ib.F_GLOC)
    if n <= 16:
        return "gen_node_kernel 5..16"
    if n <= 32:
        return "big inverse 17..32" if inverse else "gen_node_kernel 17..32"
    return "big inverse 33..64" if inverse else "big tridiagonal 33..64"


def bar(n, fid):
    if n <= 4:
        return 1e-11 if fid == ib.F_DOS_EIG else 1e-12
    return 1e-10


def params_of(fid, eta):
    return [1.0, 0.0] if fid == ib.F_LINEAR else ([0.7, -0.3] if fid == ib.F_LINEAR_X else ([eta] if fid in SWEPT else []))


def deviation(got, ref):
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


def raw_contract(abz, dev, src_level, parents, x, nnodes=None, sentinel=-777):
    """abz_contract_nodes as it is, on a slots array filled with a sentinel -> (status, message, slots)."""
    L = abz._lib
    parents = np.ascontiguousarray(parents, dtype=np.int64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    slots = np.full(max(len(x), 1), sentinel, dtype=np.int64)
    rc = L.lib().abz_contract_nodes(dev.h, src_level, parents.ctypes.data_as(L.c_i64p), x.ctypes.data_as(L.c_f64p),
                                    len(x) if nnodes is None else nnodes, slots.ctypes.data_as(L.c_i64p))
    return rc, L.lib().abz_last_error().decode("utf-8", "replace"), slots


def raw_eval(abz, dev, parents, x, fid, params, sweep, tail=None, nnodes=None, nparams=None, ncomp=None, sentinel=-777.25):
    """abz_eval_line_nodes as it is, on a values array filled with a sentinel -> (status, message, values)."""
    L = abz._lib
    parents = np.ascontiguousarray(parents, dtype=np.int64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    npar = len(params) if nparams is None else nparams
    params = np.ascontiguousarray(list(params) + [0.0] * 5, dtype=np.float64)  # (readable up to any nparams a case names)
    nc = ib.ncomp(fid, dev.s.n, dev.s.d) if ncomp is None else ncomp
    vals = np.full((max(len(x), 1), nc, 2), sentinel)
    ptail = None if tail is None else np.ascontiguousarray(tail, dtype=np.float64).ctypes.data_as(L.c_f64p)
    rc = L.lib().abz_eval_line_nodes(dev.h, parents.ctypes.data_as(L.c_i64p), x.ctypes.data_as(L.c_f64p), ptail,
                                     len(x) if nnodes is None else nnodes, fid, params.ctypes.data_as(L.c_f64p), npar, float(sweep),
                                     vals.ctypes.data_as(L.c_f64p))
    return rc, L.lib().abz_last_error().decode("utf-8", "replace"), vals


class Tree:
    """The same contraction tree on the device and in the restatement, with the coordinates of every level-1 set."""

    def __init__(self, abz, s, so, rng, n2=7, n1=40):
        self.dev, self.ref, self.d = s.device(), ib.NumpyBlocks(so), so.d
        d = so.d
        self.tails = np.zeros((1, max(d - 1, 0)))  # outer coordinates (x_2..x_d) of every level-1 set
        if d == 1:
            return
        p2, outer = np.zeros(n1, dtype=np.int64), np.zeros((n1, 0))
        if d == 3:
            x3 = rng.uniform(-1.5, 2.5, n2)
            self.both("contract_nodes", 3, np.zeros(n2, dtype=np.int64), x3)
            p2 = rng.integers(0, n2, n1)  # shuffled and repeated
            outer = x3[p2][:, None]
        x2 = rng.uniform(-1.5, 2.5, n1)
        slots = self.both("contract_nodes", 2, p2, x2)
        assert np.array_equal(slots, np.arange(n1))
        self.tails = np.concatenate([x2[:, None], outer], axis=1)

    def both(self, name, *args, **kw):
        got = getattr(self.dev, name)(*args, **kw)
        ref = getattr(self.ref, name)(*args, **kw)
        assert got.dtype == ref.dtype and np.array_equal(got, ref), (name, got, ref)
        return got

    def nodes(self, rng, nn):
        p = rng.integers(0, len(self.tails), nn) if self.d > 1 else np.zeros(nn, dtype=np.int64)
        return p, rng.uniform(-1.5, 2.5, nn)

    def check(self, fid, p, x, eta, sweep):
        """(deviation of the device values from the restatement, device values)."""
        tail = self.tails[p] if (fid == ib.F_LINEAR_X and self.d > 1) else None
        par = params_of(fid, eta)
        got = self.dev.eval_line_nodes(p, x, fid, par, sweep, tail=tail)
        ref = self.ref.eval_line_nodes(p, x, fid, par, sweep, tail=tail)
        return deviation(got, ref), got


# ---------------------------------------------------------------- a. node values against the restatement
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_node_values_match_restatement(abz, d, n):
    worst = {}
    for herm in (False, True):
        rng = np.random.default_rng(1000 * d + 10 * n + herm)
        s, so = make_series(abz, rng, d, n, herm)
        tree = Tree(abz, s, so, rng)
        ok_ids, refused = accepted(n)
        eta, sweep = float(rng.uniform(0.4, 0.8)), float(rng.uniform(-1.0, 1.0))
        for nn in ((1, 15, 16, 255, 256, 257) if n < 33 else (1, 16, 31)):
            p, x = tree.nodes(rng, nn)
            for fid in ok_ids:
                dev_, got = tree.check(fid, p, x, eta, sweep)
                b = bar(n, fid)
                key = family(n, herm, fid)
                worst[key] = max(worst.get(key, 0.0), dev_ / b)
                assert dev_ <= b, (d, n, herm, nn, NAMES[fid], dev_, b)
                if fid == ib.F_LINEAR:  # (a, b) = (1, 0): the series value itself, the contraction chain against one direct sum
                    X = np.concatenate([x[:, None], tree.tails[p]], axis=1)
                    direct = np.asarray(orc.evaluate_many(so, X))[:, 0, 0]
                    assert deviation(got[:, 0], direct) <= 1e-12, (d, nn)
            if nn == 16:
                for fid, status in refused.items():
                    tail = tree.tails[p] if d > 1 else None
                    rc, msg, vals = raw_eval(abz, tree.dev, p, x, fid, params_of(fid, eta), sweep, tail=tail)
                    assert rc == status and msg, (n, NAMES[fid], rc, msg)
                    assert np.all(vals == -777.25), (n, NAMES[fid])
        s.device().close()
    for key, w in sorted(worst.items()):
        print(f"iai-blocks a: d={d} n={n:2d} {key}: worst deviation / bar = {w:.2e}")


# ---------------------------------------------------------------- b. a node's value does not depend on its batch
@pytest.mark.parametrize("herm", [False, True])
@pytest.mark.parametrize("n", [3, 6, 12, 24, 40])
def test_node_value_does_not_depend_on_batch(abz, n, herm):
    """abz_iai_set_exchange promises a sharded solve bit-identical to the single-GPU one: every rank evaluates its own
    batches of nodes, so a node must come out the same in any batch, in any position, from sets contracted in any batch."""
    rng = np.random.default_rng(77 + n)
    s, so = make_series(abz, rng, 2, n, herm)
    dev = s.device()
    x2 = rng.uniform(-1.5, 2.5, 40)
    dev.contract_nodes(2, np.zeros(40, dtype=np.int64), x2)
    p, x = rng.integers(0, 40, 257), rng.uniform(-1.5, 2.5, 257)
    eta, sweep = 0.55, 0.2
    whole = {}
    for fid in (ib.F_TRGLOC, ib.F_GLOC):
        whole[fid] = one = dev.eval_line_nodes(p, x, fid, [eta], sweep)
        rev = dev.eval_line_nodes(p[::-1], x[::-1], fid, [eta], sweep)[::-1]
        assert np.array_equal(one, rev), (n, herm, NAMES[fid], "reversed")
        parts, i0 = [], 0
        for cnt in (1, 15, 64, 177):
            parts.append(dev.eval_line_nodes(p[i0:i0 + cnt], x[i0:i0 + cnt], fid, [eta], sweep))
            i0 += cnt
        assert i0 == 257 and np.array_equal(one, np.concatenate(parts)), (n, herm, NAMES[fid], "split")
    # the level-1 sets made in other batches: 13 + 27 nodes, the second batch appended behind the first
    dev.release_level(2)
    assert np.array_equal(dev.contract_nodes(2, np.zeros(13, dtype=np.int64), x2[:13]), np.arange(13))
    assert np.array_equal(dev.contract_nodes(2, np.zeros(27, dtype=np.int64), x2[13:]), np.arange(13, 40))
    for fid in (ib.F_TRGLOC, ib.F_GLOC):
        assert np.array_equal(whole[fid], dev.eval_line_nodes(p, x, fid, [eta], sweep)), (n, herm, NAMES[fid], "contraction batches")
    dev.close()


# ---------------------------------------------------------------- c. appending and growth
@pytest.mark.parametrize("grow_level", [1, 2])
def test_appended_slots_survive_pool_growth(abz, grow_level):
    """A second contract_nodes call that outgrows the level's pool while 3 slots are live: the library allocates a larger
    buffer, copies the live sets device to device and swaps the buffers.  grow_level 1: the level-1 pool (src_level 2);
    grow_level 2: the level-2 pool (src_level 3), so that the parents of the level-1 contraction point into the grown pool."""
    rng = np.random.default_rng(31 + grow_level)
    n, d = 3, 3
    s, so = make_series(abz, rng, d, n, False, dims=(4, 2, 3))
    dev, ref = s.device(), ib.NumpyBlocks(so)
    Lrow = int(np.prod(so.dims[:grow_level])) * n * n  # complex numbers per set of the growing level
    # the first request reserves 3 sets + 25 % + 256 B, and a recycled block may be twice that + 4 KB: the second request
    # is more than 4 times the largest capacity the first can have got, and at least 600 nodes
    first_cap = 2 * (3 * 16 * Lrow * 5 // 4 + 256) + 4096
    N = max(600, -(-4 * first_cap // (16 * Lrow)))
    eta, sweep = 0.6, -0.35
    xe = rng.uniform(-1.5, 2.5, 3)

    def both(name, *args):
        got, want = getattr(dev, name)(*args), getattr(ref, name)(*args)
        assert np.array_equal(got, want), (name, got, want)
        return got

    if grow_level == 1:
        both("contract_nodes", 3, [0], rng.uniform(-1.5, 2.5, 1))
        first = both("contract_nodes", 2, [0, 0, 0], rng.uniform(-1.5, 2.5, 3))
        assert np.array_equal(first, [0, 1, 2])
        before = dev.eval_line_nodes(first, xe, ib.F_GLOC, [eta], sweep)
        new = both("contract_nodes", 2, np.zeros(N, dtype=np.int64), rng.uniform(-1.5, 2.5, N))
        assert np.array_equal(new, np.arange(3, 3 + N))
        after = dev.eval_line_nodes(first, xe, ib.F_GLOC, [eta], sweep)
        last = new[-3:]
    else:
        first = both("contract_nodes", 3, [0, 0, 0], rng.uniform(-1.5, 2.5, 3))
        assert np.array_equal(first, [0, 1, 2])
        x2 = rng.uniform(-1.5, 2.5, 3)
        before = dev.eval_line_nodes(both("contract_nodes", 2, first, x2), xe, ib.F_GLOC, [eta], sweep)
        new = both("contract_nodes", 3, np.zeros(N, dtype=np.int64), rng.uniform(-1.5, 2.5, N))
        assert np.array_equal(new, np.arange(3, 3 + N))
        again = both("contract_nodes", 2, first, x2)  # from the copies of slots 0..2 in the grown level-2 pool
        assert np.array_equal(again, [3, 4, 5])
        after = dev.eval_line_nodes(again, xe, ib.F_GLOC, [eta], sweep)
        last = both("contract_nodes", 2, new[-3:], rng.uniform(-1.5, 2.5, 3))
    assert np.array_equal(before, after), "sets made before the pool grew changed"
    dev_first = deviation(before, ref.eval_line_nodes([0, 1, 2], xe, ib.F_GLOC, [eta], sweep))
    got = dev.eval_line_nodes(last, xe, ib.F_GLOC, [eta], sweep)
    dev_last = deviation(got, ref.eval_line_nodes(last, xe, ib.F_GLOC, [eta], sweep))
    print(f"iai-blocks c: level-{grow_level} pool, N = {N}: first slots {dev_first:.2e}, last slots {dev_last:.2e} (bar 1e-12)")
    assert dev_first <= 1e-12 and dev_last <= 1e-12
    dev.close()


# ---------------------------------------------------------------- d. release, and mixing with the library's own solve
def lib_iai_solve(abz, dev, fid, params, sweep, abstol):
    """abz_iai_solve on the unit cube, scalar refinement -> (value [ncomp], err, numevals)."""
    L = abz._lib
    d, n = dev.s.d, dev.s.n
    out = np.full((ib.ncomp(fid, n, d), 2), np.nan)
    err, nev, npan = C.c_double(0.0), C.c_int64(0), C.c_int64(0)
    _, pa = L.f64(np.zeros(d))
    _, pb = L.f64(np.ones(d))
    par = np.ascontiguousarray(params, dtype=np.float64)
    L.check(L.lib().abz_iai_solve(dev.h, L.LIMS_CUBIC, pa, pb, fid, par.ctypes.data_as(L.c_f64p), len(par), float(sweep), float(abstol),
                                  -1.0, 2 ** 62, 0, out.ctypes.data_as(L.c_f64p), C.byref(err), C.byref(nev), None, 0, C.byref(npan)))
    return out.view(np.complex128).reshape(-1).copy(), err.value, nev.value


def test_release_and_mixing_with_the_library_solve(abz):
    """A Hermitian 3-band series: abz_iai_solve runs on packed coefficient rows in the same pools the blocks use unpacked."""
    rng = np.random.default_rng(8)
    c, first = _herm_series(rng, (3, 3, 3), 3, 1.0 / np.sqrt(3))
    x3, x2, x1 = rng.uniform(-1.5, 2.5, 4), rng.uniform(-1.5, 2.5, 6), rng.uniform(-1.5, 2.5, 9)
    p2, p1 = np.array([3, 0, 0, 2, 1, 3]), np.array([5, 0, 0, 1, 4, 2, 3, 3, 5])
    eta, sweep = 0.3, 0.1

    def blocks(dev):
        assert np.array_equal(dev.contract_nodes(3, np.zeros(4, dtype=np.int64), x3), np.arange(4))
        assert np.array_equal(dev.contract_nodes(2, p2, x2), np.arange(6))
        return [dev.eval_line_nodes(p1, x1, fid, [eta], sweep) for fid in (ib.F_GLOC, ib.F_DOS, ib.F_DOS_EIG)]

    s = abz.FourierSeries(c, period=1.0, first=first, ndim=3)
    dev = s.device()
    assert dev.hermitian()
    v1 = blocks(dev)
    so = orc.FourierSeries(c, period=1.0, first=first, ndim=3)
    refb = ib.NumpyBlocks(so)
    refb.contract_nodes(3, np.zeros(4, dtype=np.int64), x3)
    refb.contract_nodes(2, p2, x2)
    assert deviation(v1[0], refb.eval_line_nodes(p1, x1, ib.F_GLOC, [eta], sweep)) <= 1e-12
    dev.release_level(2)  # the level-1 sets only
    assert np.array_equal(dev.contract_nodes(2, [1], [0.3]), [0])
    assert np.array_equal(dev.contract_nodes(3, [0], [0.3]), [4])
    dev.release_level(3)
    assert np.array_equal(dev.contract_nodes(3, [0, 0], [0.3, 0.4]), [0, 1])  # release_level(d): from 0 again
    dev.release_level(3)
    v2 = blocks(dev)
    assert all(np.array_equal(a, b) for a, b in zip(v1, v2))
    solved = lib_iai_solve(abz, dev, ib.F_DOS, [eta], sweep, 1e-2)
    rc, msg, _ = raw_eval(abz, dev, [0], [0.0], ib.F_DOS, [eta], sweep)  # the solve invalidated the blocks' slots
    assert rc == abz._lib.ERR_ARG and "0 live" in msg
    v3 = blocks(dev)  # fresh blocks after the solve, slots from 0
    assert all(np.array_equal(a, b) for a, b in zip(v1, v3))
    solved_again = lib_iai_solve(abz, dev, ib.F_DOS, [eta], sweep, 1e-2)
    # the same solve on a device series that never saw a building-block call
    s0 = abz.FourierSeries(c, period=1.0, first=first, ndim=3)
    alone = lib_iai_solve(abz, s0.device(), ib.F_DOS, [eta], sweep, 1e-2)
    assert np.array_equal(solved[0], alone[0]) and solved[1:] == alone[1:]
    assert np.array_equal(solved_again[0], alone[0]) and solved_again[1:] == alone[1:]
    assert alone[2] > 15 ** 3
    dev.close()
    s0.device().close()


# ---------------------------------------------------------------- e. the documented use case: a host-driven adaptive loop
@pytest.mark.parametrize("n,dims,eta,omega,abstol,seed", DRIVER_CASES + [(6, (3, 3), 0.3, 0.3, 1e-2, 9)])
def test_host_driven_nested_gk_on_device_blocks(abz, n, dims, eta, omega, abstol, seed):
    d = len(dims)
    c, first, so = driver_case(n, dims, seed)
    s = abz.FourierSeries(c, period=1.0, first=first, ndim=d)
    dev = s.device()
    lims = orc.CubicLimits(np.zeros(d), np.ones(d))
    I, E, nev = ib.nested_gk(dev, d, lims, ib.F_DOS, [eta], omega, abstol=abstol)
    I0, E0, nev0 = orc.nested_quad(so, lims, orc.f_dos(eta, omega), abstol=abstol)
    lib_I, lib_E, lib_nev = lib_iai_solve(abz, dev, ib.F_DOS, [eta], omega, abstol)
    rel, rel_lib = abs(I[0] - I0) / abs(I0), abs(I[0] - lib_I[0]) / abs(I0)
    print(f"iai-blocks e: n={n} dims={dims}: numevals {nev} (oracle {nev0}, abz_iai_solve {lib_nev}); "
          f"blocks vs oracle {rel:.2e}, blocks vs abz_iai_solve {rel_lib:.2e} (bar 1e-9)")
    assert nev == nev0 and nev > 15 ** d
    assert rel <= 1e-9
    assert lib_nev == nev and rel_lib <= 1e-9
    dev.close()


# ---------------------------------------------------------------- f. refusals
def test_refusals_leave_outputs_and_slot_counts_untouched(abz):
    """Every call below is refused by a host-side check of abz_contract_nodes / abz_eval_line_nodes before any device
    work (iai_host.cpp: check_node_parents and the ABZ_REQUIRE lines above it)."""
    L = abz._lib
    rng = np.random.default_rng(4)
    s, so = make_series(abz, rng, 3, 1, False)
    dev, ref = s.device(), ib.NumpyBlocks(so)
    for b in (dev, ref):
        assert np.array_equal(b.contract_nodes(3, [0, 0], [0.3, 1.4]), [0, 1])
        assert np.array_equal(b.contract_nodes(2, [1, 0, 1], [-0.2, 0.9, 2.1]), [0, 1, 2])

    def refused_contract(what, needle, *args, **kw):
        rc, msg, slots = raw_contract(abz, dev, *args, **kw)
        assert rc == L.ERR_ARG and msg and needle in msg, (what, rc, msg)
        assert np.all(slots == -777), what

    def refused_eval(what, needle, *args, **kw):
        rc, msg, vals = raw_eval(abz, dev, *args, **kw)
        assert rc == L.ERR_ARG and msg and needle in msg, (what, rc, msg)
        assert np.all(vals == -777.25), what

    refused_contract("parent = live count", "parents[1] = 2", 2, [0, 2, 1], [0.1, 0.2, 0.3])
    refused_contract("live count in the message", "2 live", 2, [0, 2, 1], [0.1, 0.2, 0.3])
    refused_contract("negative parent", "parents[0] = -1", 2, [-1], [0.1])
    refused_contract("non-zero parent at level d", "parents[1] = 1", 3, [0, 1], [0.1, 0.2])
    refused_contract("nnodes = -1", "negative", 2, [0], [0.1], nnodes=-1)
    refused_contract("src_level 1", "src_level", 1, [0], [0.1])
    refused_contract("src_level d + 1", "src_level", 4, [0], [0.1])
    refused_eval("parent = live count", "parents[2] = 3", [0, 1, 3], [0.1, 0.2, 0.3], ib.F_DOS, [0.5], 0.1)
    refused_eval("live count in the message", "3 live", [0, 1, 3], [0.1, 0.2, 0.3], ib.F_DOS, [0.5], 0.1)
    refused_eval("negative parent", "parents[0] = -5", [-5], [0.1], ib.F_DOS, [0.5], 0.1)
    refused_eval("nnodes = -1", "negative", [0], [0.1], ib.F_DOS, [0.5], 0.1, nnodes=-1)
    refused_eval("F_LINEAR_X without tail", "tail", [0], [0.1], ib.F_LINEAR_X, [1.0, 0.0], 0.0)
    refused_eval("nparams = 5", "nparams", [0], [0.1], ib.F_DOS, [0.5], 0.1, nparams=5)
    refused_eval("unknown integrand", "integrand", [0], [0.1], 7, [0.5], 0.1, ncomp=1, nparams=1)
    # nnodes = 0 is fine and does nothing
    rc, _, slots = raw_contract(abz, dev, 2, [0], [0.1], nnodes=0)
    assert rc == 0 and np.all(slots == -777)
    rc, _, vals = raw_eval(abz, dev, [0], [0.1], ib.F_DOS, [0.5], 0.1, nnodes=0)
    assert rc == 0 and np.all(vals == -777.25)
    # the counts did not move: the next valid calls number from where the last valid ones stopped
    for b in (dev, ref):
        assert np.array_equal(b.contract_nodes(3, [0], [0.6]), [2])
        assert np.array_equal(b.contract_nodes(2, [2, 0], [0.5, 0.7]), [3, 4])
    # a slot that is stale after release_level
    for b in (dev, ref):
        b.release_level(2)
    refused_eval("stale level-1 slot", "0 live", [0], [0.1], ib.F_DOS, [0.5], 0.1)
    for b in (dev, ref):
        b.release_level(3)
    refused_contract("stale level-2 slot", "0 live", 2, [0], [0.1])
    with pytest.raises(ValueError):  # the mirror turns ABZ_ERR_ARG into ValueError like every wrapper
        dev.contract_nodes(2, [0], [0.1])
    # d = 1: nothing to contract, and the only parent is 0
    s1, so1 = make_series(abz, rng, 1, 1, False)
    dev1 = s1.device()
    for lvl in (1, 2):
        rc, msg, slots = raw_contract(abz, dev1, lvl, [0], [0.1])
        assert rc == L.ERR_ARG and "src_level" in msg and np.all(slots == -777)
    rc, msg, vals = raw_eval(abz, dev1, [0, 1], [0.1, 0.2], ib.F_DOS, [0.5], 0.1)
    assert rc == L.ERR_ARG and "parents[1] = 1" in msg and np.all(vals == -777.25)
    dev1.close()
    # a valid sequence afterwards still meets the bar of section a
    p2, x2 = np.array([0, 0, 0]), np.array([0.3, -1.1, 2.2])
    p1, x1 = np.array([2, 0, 1, 1]), np.array([0.2, 1.7, -0.4, 0.9])
    x = rng.uniform(-1.5, 2.5, 17)
    p = rng.integers(0, 4, 17)
    for b in (dev, ref):
        assert np.array_equal(b.contract_nodes(3, p2, x2), [0, 1, 2])
        assert np.array_equal(b.contract_nodes(2, p1, x1), [0, 1, 2, 3])
    for fid in (ib.F_LINEAR, ib.F_GLOC):
        par = params_of(fid, 0.5)
        assert deviation(dev.eval_line_nodes(p, x, fid, par, 0.1), ref.eval_line_nodes(p, x, fid, par, 0.1)) <= 1e-12
    dev.close()

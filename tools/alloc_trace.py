"""Allocation trace: a fixed walk over the entry points that own device memory, all five numbers of abz_mem_info (live,
cached, context scratch, pinned host bytes, live blocks) printed after every call.  Run it on two builds of the library in
fresh processes (ABZ_LIB=<other libabzhip.so> selects one) and diff the outputs: an ownership change that keeps the
allocator's requests -- sizes, order, frees -- leaves them identical.
    python tools/alloc_trace.py > new.txt;  ABZ_LIB=/path/to/parent/libabzhip.so python tools/alloc_trace.py > parent.txt"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz

L = abz._lib
lib = L.lib()
ctx = L.Context.default()
step = [0]


def mark(what):
    step[0] += 1
    print(f"{step[0]:3d} {what:58s} " + " ".join(f"{v:12d}" for v in ctx.mem_info()), flush=True)


def series(n, d, seed):
    rng = np.random.default_rng(seed)
    dims = (3,) * d
    c = (rng.standard_normal(dims + (n, n)) + 1j * rng.standard_normal(dims + (n, n))) / np.sqrt(n)
    flip = c[tuple(slice(None, None, -1) for _ in dims)]
    c = 0.5 * (c + np.conj(np.swapaxes(flip, -1, -2)))
    return abz.FourierSeries(c, period=1.0, first=(-1,) * d, ndim=d)


mark("context")
cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
npt = 12
for n in (3, 6):
    s = series(n, 3, n)
    dev = s.device()
    mark(f"n={n} series")
    full = abz.DeviceRule(dev, npt, None, L.WANT_H | L.WANT_EIG)
    mark(f"n={n} full rule H+E")
    vel = abz.DeviceRule(dev, npt, None, L.WANT_EIG | L.WANT_VEL)
    mark(f"n={n} full rule E+V (fused build)")
    velh = abz.DeviceRule(dev, npt, None, L.WANT_H | L.WANT_EIG | L.WANT_VEL)
    mark(f"n={n} full rule H+E+V (temporaries of the velocity build)")
    sym = abz.DeviceRule(dev, npt, cub.syms, L.WANT_H | L.WANT_EIG)
    mark(f"n={n} symmetric rule")
    sym2 = abz.DeviceRule(dev, npt, cub.syms, L.WANT_EIG)
    mark(f"n={n} symmetric rule again (cached tables)")
    idx, w = abz.symptr_rule(npt, 3, cub.syms)
    mark(f"n={n} symptr_rule_device")
    lst = C.c_void_p()
    L.check(lib.abz_ptr_rule_build(dev.h, npt, len(w), idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_H, C.byref(lst)))
    mark(f"n={n} explicit node list rule")
    slab = C.c_void_p()
    L.check(lib.abz_ptr_rule_build_slab(dev.h, npt, 3, 7, L.WANT_EIG, C.byref(slab)))
    mark(f"n={n} slab rule")
    L.check(lib.abz_rule_ltm_halo(slab))
    mark(f"n={n} halo")
    dev.update(s.c * 1.5)
    mark(f"n={n} series update")
    for name, r in (("full", full), ("vel", vel), ("velh", velh), ("sym", sym)):
        r.rebuild()
        mark(f"n={n} rebuild {name}")
    L.check(lib.abz_rule_rebuild(slab))
    mark(f"n={n} rebuild slab + halo")
    om = np.linspace(-1.0, 1.0, 5)
    full.reduce(L.F_DOS, (0.2,), om)
    mark(f"n={n} reduce full")
    sym.reduce(L.F_TRGLOC, (0.2,), om)
    mark(f"n={n} reduce symmetric")
    dev.ptr_sum(npt, L.F_DOS, (0.2,), om)
    mark(f"n={n} ptr_sum")
    dev.eval_nodes(np.random.default_rng(1).random((300, 3)), want=3)
    mark(f"n={n} eval_nodes")
    for keepmost in (2, 0):
        out, err = np.zeros(2 * len(om)), np.zeros(len(om))
        nev, npo = np.zeros(len(om), dtype=np.int64), np.zeros(len(om), dtype=np.int32)
        eta = np.array([0.3])
        L.check(lib.abz_autoptr_solve_many(dev.h, None, 0, L.F_DOS, eta.ctypes.data_as(L.c_f64p), 1, om.ctypes.data_as(L.c_f64p), len(om),
                                           6, 2, 1e-3, 0.0, 20000, keepmost, 1.0, out.ctypes.data_as(L.c_f64p), err.ctypes.data_as(L.c_f64p),
                                           nev.ctypes.data_as(L.c_i64p), npo.ctypes.data_as(L.c_i32p)))
        mark(f"n={n} autoptr keepmost={keepmost} (to npt {npo.max()})")
    S = np.ascontiguousarray(np.rint(np.asarray(cub.syms)).astype(np.int32).reshape(-1, 3, 3))
    L.check(lib.abz_autoptr_solve_many(dev.h, S.ctypes.data_as(L.c_i32p), len(S), L.F_DOS, eta.ctypes.data_as(L.c_f64p), 1,
                                       om.ctypes.data_as(L.c_f64p), len(om), 6, 2, 1e-3, 0.0, 20000, 2, 1.0, out.ctypes.data_as(L.c_f64p),
                                       err.ctypes.data_as(L.c_f64p), nev.ctypes.data_as(L.c_i64p), npo.ctypes.data_as(L.c_i32p)))
    mark(f"n={n} autoptr symmetric (to npt {npo.max()})")
    dev.drop_rules()
    mark(f"n={n} drop kept rules")
    eig = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    mark(f"n={n} full rule E")
    eig.ltm_elements(np.random.default_rng(2).standard_normal((2, npt ** 3, n)))
    mark(f"n={n} ltm elements attached")
    eig.ltm_orbitals()
    mark(f"n={n} ltm orbitals (transient H rule)")
    eig.ltm_elements(None)
    mark(f"n={n} ltm elements dropped")
    unf = sym2.unfold()
    mark(f"n={n} unfold")
    unf.rebuild()
    mark(f"n={n} unfold refresh")
    short, again = C.c_void_p(), C.c_void_p()  # a node list that misses an orbit: refused after the map was made
    L.check(lib.abz_ptr_rule_build(dev.h, npt, len(w) - 1, idx.ctypes.data_as(L.c_i32p), w.ctypes.data_as(L.c_i64p), L.WANT_EIG, C.byref(short)))
    rc = lib.abz_rule_ltm_unfold(short, S.ctypes.data_as(L.c_i32p), len(S), C.byref(again))
    mark(f"n={n} unfold refused (rc {rc})")
    L.check(lib.abz_rule_destroy(short))
    solver = abz.IntegralSolver(abz.FourierIntegrand(abz.DOSIntegrand(), s, 0.4), abz.load_bz(abz.FBZ(), np.eye(3)), abz.IAI(), abstol=1e-2)
    solver(0.1)
    mark(f"n={n} IAI solve")
    dev.contract_nodes(3, np.zeros(4, dtype=np.int64), np.linspace(0.1, 0.4, 4))
    mark(f"n={n} contract_nodes 4")
    dev.contract_nodes(3, np.zeros(60, dtype=np.int64), np.linspace(0.1, 0.9, 60))
    mark(f"n={n} contract_nodes 60 (pool grows)")
    dev.release_level(3)
    mark(f"n={n} release_level")
    for name, r in (("unfolded", unf), ("eig", eig), ("sym2", sym2), ("sym", sym), ("velh", velh), ("vel", vel), ("full", full)):
        r.close()
        mark(f"n={n} destroy {name}")
    for name, h in (("slab", slab), ("list", lst)):
        L.check(lib.abz_rule_destroy(h))
        mark(f"n={n} destroy {name}")
    del solver
    dev.close()
    mark(f"n={n} series destroyed")
ctx2 = L.Context()
mark("second context")
ctx2.close()
mark("second context destroyed")

"""Tetrahedron DOS from irreducible nodes against the full-grid path, same series, grid and energies.
  full:       eigenvalue build of the whole grid (abz_ptr_rule_build(WANT_EIG) refilled by abz_rule_rebuild) + LTM scan -- the yardstick;
  symmetric:  eigenvalue build of the irreducible nodes (abz_ptr_rule_build_sym refilled by abz_rule_rebuild) + the gather
              (abz_rule_ltm_unfold into the rule it made, its orbit map reused) + the same scan;
  first call: abz_rule_ltm_unfold with *out = NULL (allocation, orbit map, gather), created and destroyed per call.
Wall times are host clocks around calls that end in a stream synchronisation, the median of `--repeats` repeats of `--calls`
calls each after a warm-up, profiler off; the kernel times beside them come from the library's own HIP events (ABZ_K_LTM for
map, gather and scans, ABZ_K_CONTRACT + ABZ_K_EVAL + ABZ_K_EIG for a build) in a separate pass.  The map's kernel time is
(first call) - (gather).  The synthetic series are the average of synthetic_wannier(n, rmax=2, seed=7) over the 48 signed
permutations of the lattice axes (tests/unfold_numpy.py), which makes the cubic operations symmetries of H.
Usage: time_ltm_sym.py [--cases svo:24 svo:48 svo:150 syn16:48 syn32:48 syn64:24] [--nE 32 256] [--repeats 3] [--calls 10] [--json FILE]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L
from unfold_numpy import symmetrise_coefficients  # one definition of "the cubic-symmetrised synthetic series"

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["svo:24", "svo:48", "svo:150", "syn16:48", "syn32:48", "syn64:24"])
ap.add_argument("--nE", nargs="+", type=int, default=[32, 256])
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--json", default=None)
args = ap.parse_args()


def make(name):
    if name == "svo":
        return abz.load_w90_series(os.path.join(ROOT, "tests", "golden", "svo_hr.dat.gz"))
    s = abz.synthetic_wannier(int(name[3:]), rmax=2, seed=7)
    return abz.FourierSeries(symmetrise_coefficients(s.c, (-2, -2, -2)), period=1.0, first=-2, ndim=3)


def median_ms(fn, ctx):
    """median over the repeats of the mean wall time of a call, ms"""
    fn(); ctx.sync()
    ts = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(args.calls): fn()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0) / args.calls)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernel_ms(fn, ctx, kids):
    """mean time per call of the call's kernels from the library's events, ms"""
    ctx.prof_enable(True, kernels=kids); ctx.prof_reset()
    for _ in range(args.calls): fn()
    ctx.sync()
    ms = sum(ctx.prof_read(k)[0] for k in kids); ctx.prof_enable(False)
    return ms / args.calls


BUILD = [L.K_CONTRACT, L.K_EVAL, L.K_EIG]
cubic = abz.load_bz(abz.CubicSymIBZ(), np.eye(3)).syms
S = np.ascontiguousarray(np.rint(np.asarray(cubic)).astype(np.int32))
pS = S.ctypes.data_as(L.c_i32p)
rows = []
for case in args.cases:
    name, npt = case.split(":"); npt = int(npt)
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    full = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    src = abz.DeviceRule(dev, npt, cubic, L.WANT_EIG)
    unf = src.unfold()
    for _ in range(3): full.rebuild(); src.rebuild()
    ctx.sync()

    def gather():
        L.check(L.lib().abz_rule_ltm_unfold(src._h, pS, len(S), C.byref(unf._hbox)))

    def first():
        h = C.c_void_p()
        L.check(L.lib().abz_rule_ltm_unfold(src._h, pS, len(S), C.byref(h)))
        L.check(L.lib().abz_rule_destroy(h))

    t = {"full_build": median_ms(full.rebuild, ctx), "sym_build": median_ms(src.rebuild, ctx), "gather": median_ms(gather, ctx),
         "first": median_ms(first, ctx)}
    k = {"full_build": kernel_ms(full.rebuild, ctx, BUILD), "sym_build": kernel_ms(src.rebuild, ctx, BUILD),
         "gather": kernel_ms(gather, ctx, [L.K_LTM]), "first": kernel_ms(first, ctx, [L.K_LTM])}
    ef, eu = full.export(x=False, w=False, eig=True)["eig"], unf.export(x=False, w=False, eig=True)["eig"]
    lo, hi = float(ef.min()), float(ef.max())
    for nE in args.nE:
        Es = np.linspace(lo, hi, nE)
        row = {"series": name, "bands": n, "npt": npt, "nE": nE, "nodes": src.nk, "grid": unf.nk, "eig_max_dev": float(np.abs(ef - eu).max())}
        for key in t:
            row[key + "_ms"], row[key + "_minmax_ms"], row[key + "_kernel_ms"] = t[key][0], t[key][1:], k[key]
        row["map_kernel_ms"] = k["first"] - k["gather"]
        for key, rule in (("scan_full", full), ("scan_unf", unf)):
            fn = lambda: rule.ltm(Es)
            med, lo_, hi_ = median_ms(fn, ctx)
            row[key + "_ms"], row[key + "_minmax_ms"], row[key + "_kernel_ms"] = med, (lo_, hi_), kernel_ms(fn, ctx, [L.K_LTM])
        row["full_total_ms"] = row["full_build_ms"] + row["scan_full_ms"]
        row["sym_total_ms"] = row["sym_build_ms"] + row["gather_ms"] + row["scan_unf_ms"]
        row["sym_first_total_ms"] = row["sym_build_ms"] + row["first_ms"] + row["scan_unf_ms"]
        row["g_max_dev"] = float(np.abs(full.ltm(Es) - unf.ltm(Es)).max())
        rows.append(row)
        print(f"LTMSYM {name} n={n} npt={npt} nE={nE} nodes {src.nk}/{unf.nk}: full build {row['full_build_ms']:.4f} ms (kernels "
              f"{row['full_build_kernel_ms']:.4f}) + scan {row['scan_full_ms']:.4f} = {row['full_total_ms']:.4f} ms | sym build "
              f"{row['sym_build_ms']:.4f} (kernels {row['sym_build_kernel_ms']:.4f}) + gather {row['gather_ms']:.4f} (kernel "
              f"{row['gather_kernel_ms']:.4f}) + scan {row['scan_unf_ms']:.4f} = {row['sym_total_ms']:.4f} ms | first unfold "
              f"{row['first_ms']:.4f} ms (kernels {row['first_kernel_ms']:.4f}: map {row['map_kernel_ms']:.4f}) -> first total "
              f"{row['sym_first_total_ms']:.4f} ms | eig dev {row['eig_max_dev']:.2e} g dev {row['g_max_dev']:.2e}", flush=True)
    unf.close(); src.close(); full.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)

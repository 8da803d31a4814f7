"""Linear tetrahedron DOS against GGR on the same series, grid and energies: eigenvalue build (abz_ptr_rule_build(WANT_EIG)
refilled by abz_rule_rebuild), LTM scan for g(E) and for N(E) (abz_rule_ltm), and the yardstick, GGR build (WANT_EIG | WANT_VEL)
and scan (abz_rule_ggr).  Wall times are host clocks around calls that end in a stream synchronisation, the median of
`--repeats` repeats of `--calls` calls each, profiler off; the kernel times beside them come from the library's own HIP
events (ABZ_K_LTM / ABZ_K_GGR) in a separate pass.  Algorithmic bytes of a scan: n npt^d 8 B of eigenvalues, read once if
the neighbour lines hit in L2.
Usage: time_ltm.py [--series svo syn16 syn32] [--npt 24 48] [--nE 32 256] [--repeats 3] [--calls 10] [--json FILE]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--series", nargs="+", default=["svo"])
ap.add_argument("--npt", nargs="+", type=int, default=[24, 48])
ap.add_argument("--nE", nargs="+", type=int, default=[32, 256])
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--json", default=None)
args = ap.parse_args()


def make(name):
    if name == "svo":
        return abz.load_w90_series(os.path.join(ROOT, "tests", "golden", "svo_hr.dat.gz"))
    return abz.synthetic_wannier(int(name[3:]), rmax=2, seed=7)


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


def kernel_ms(fn, ctx, kid):
    """mean time of the call's kernels from the library's events, ms"""
    ctx.prof_enable(True, kernels=[kid]); ctx.prof_reset()
    for _ in range(args.calls): fn()
    ctx.sync()
    ms, n = ctx.prof_read(kid); ctx.prof_enable(False)
    return ms / max(n, 1)


rows = []
for name in args.series:
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    for npt in args.npt:
        re_ = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
        rg = abz.DeviceRule(dev, npt, None, L.WANT_EIG | L.WANT_VEL)
        for _ in range(3): re_.rebuild(); rg.rebuild()
        ctx.sync()
        build_e = median_ms(re_.rebuild, ctx)
        build_g = median_ms(rg.rebuild, ctx)
        lo, hi = (10.0, 15.0) if name == "svo" else (-2.5, 2.5)
        for nE in args.nE:
            Es = np.linspace(lo, hi, nE)
            row = {"series": name, "bands": n, "npt": npt, "nE": nE, "eig_build_ms": build_e[0], "eig_build_minmax_ms": build_e[1:],
                   "ggr_build_ms": build_g[0], "ggr_build_minmax_ms": build_g[1:]}
            for key, fn, kid in (("ltm_g", lambda: re_.ltm(Es), L.K_LTM), ("ltm_N", lambda: re_.ltm(Es, states=True), L.K_LTM),
                                 ("ggr_scan", lambda: rg.ggr(Es), L.K_GGR)):
                med, lo_, hi_ = median_ms(fn, ctx)
                row[key + "_ms"], row[key + "_minmax_ms"], row[key + "_kernel_ms"] = med, (lo_, hi_), kernel_ms(fn, ctx, kid)
            alg_bytes = n * npt ** s.d * 8
            row["alg_bytes"] = alg_bytes
            row["ltm_g_GBps"] = alg_bytes / (row["ltm_g_kernel_ms"] * 1e-3) / 1e9
            row["ltm_total_ms"] = row["eig_build_ms"] + row["ltm_g_ms"]
            row["ggr_total_ms"] = row["ggr_build_ms"] + row["ggr_scan_ms"]
            g = re_.ltm(Es)
            row["sum_g"] = float(g.sum())
            rows.append(row)
            print(f"LTM {name} n={n} npt={npt} nE={nE}: eig build {row['eig_build_ms']:.4f} ms  ltm g {row['ltm_g_ms']:.4f} ms (kernels "
                  f"{row['ltm_g_kernel_ms']:.4f})  ltm N {row['ltm_N_ms']:.4f} ms (kernels {row['ltm_N_kernel_ms']:.4f})  | GGR build "
                  f"{row['ggr_build_ms']:.4f} ms  scan {row['ggr_scan_ms']:.4f} ms (kernels {row['ggr_scan_kernel_ms']:.4f})  | build+scan LTM "
                  f"{row['ltm_total_ms']:.4f} vs GGR {row['ggr_total_ms']:.4f} ms  | {alg_bytes / 1e6:.2f} MB alg, {row['ltm_g_GBps']:.1f} GB/s over "
                  f"kernel time  sum g={row['sum_g']:.9f}", flush=True)
        re_.close(); rg.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)

"""LTM on slabs of the grid, one-GPU shard timings: for every workload the full job (eigenvalue build by abz_rule_rebuild + g(E)
scan by abz_rule_ltm) on the whole grid, then, for W = 2, 4, 8 ranks, every rank's job one after another on this one GPU:
slab build + halo build (one abz_rule_rebuild refills both) + scan of the slab's cells.  Reported per W: the slowest rank --
what a W-GPU solve waits for before its all-reduce, which is not part of this -- the speed-up over the full job, and the
halo's share of that rank's time (the refill of the halo plane alone, a second abz_rule_ltm_halo, over the rank's job).
Wall times are host clocks around calls that end in a stream synchronisation (the scan delivers its result to the host), the
median of `--repeats` repeats of `--calls` calls each, profiler off.
Usage: time_ltm_slab.py [--work svo:150 syn16:48 syn32:48] [--nE 32 256] [--world 2 4 8] [--repeats 3] [--calls 10] [--json FILE]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--work", nargs="+", default=["svo:150", "syn16:48", "syn32:48"], help="series:npt")
ap.add_argument("--nE", nargs="+", type=int, default=[32, 256])
ap.add_argument("--world", nargs="+", type=int, default=[2, 4, 8])
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
    return float(np.median(ts))


rows = []
for work in args.work:
    name, npt = work.split(":")
    npt = int(npt)
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    lo, hi = (10.0, 15.0) if name == "svo" else (-2.5, 2.5)
    full = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    for nE in args.nE:
        Es = np.linspace(lo, hi, nE)
        g_full = full.ltm(Es)
        row = {"series": name, "bands": n, "npt": npt, "nE": nE,
               "full_ms": median_ms(lambda: (full.rebuild(), full.ltm(Es)), ctx), "full_scan_ms": median_ms(lambda: full.ltm(Es), ctx)}
        line = f"LTM slabs {name} n={n} npt={npt} nE={nE}: full build+scan {row['full_ms']:.4f} ms (scan {row['full_scan_ms']:.4f})"
        for W in args.world:
            ranks, total = [], np.zeros(nE)
            for r in range(W):
                dev.kshard, dev.allreduce = (r, W), (lambda a: a)
                try:
                    rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
                    rule.ltm_halo()
                    total += rule.ltm(Es)
                    job = median_ms(lambda: (rule.rebuild(), rule.ltm(Es)), ctx)
                    halo = median_ms(lambda: L.check(L.lib().abz_rule_ltm_halo(rule._h)), ctx)
                    scan = median_ms(lambda: rule.ltm(Es), ctx)
                    ranks.append({"rank": r, "planes": rule.nk_local // npt ** (s.d - 1), "job_ms": job, "halo_ms": halo, "scan_ms": scan})
                    rule.close()
                finally:
                    dev.kshard, dev.allreduce = None, None
            slow = max(ranks, key=lambda q: q["job_ms"])
            dev_ = float(np.abs(total - g_full).max() / max(1.0, np.abs(g_full).max()))
            row[f"W{W}"] = {"ranks": ranks, "slowest_ms": slow["job_ms"], "halo_share": slow["halo_ms"] / slow["job_ms"],
                            "speedup": row["full_ms"] / slow["job_ms"], "sum_vs_full": dev_}
            line += (f"  | W={W}: slowest rank {slow['job_ms']:.4f} ms (scan {slow['scan_ms']:.4f}, halo {slow['halo_ms']:.4f} = "
                     f"{100 * slow['halo_ms'] / slow['job_ms']:.1f} %), x{row['full_ms'] / slow['job_ms']:.2f}, sum of slabs off by {dev_:.1e}")
        rows.append(row)
        print(line, flush=True)
    full.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)

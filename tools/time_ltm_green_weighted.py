"""Tetrahedron Green's function with matrix elements (abz_rule_ltm_green_weighted) against the trace (abz_rule_ltm_green) on the
same eigenvalue rule and the same values of z: the trace, the weighted call with the energy as the element (one component), the
weighted call with the device orbital weights of all orbitals (SVO: three components, groups 2 + 1), and one single-component
call per orbital.  One session; every call is warmed up first; the times are the kernels' own, from the library's HIP events
(ABZ_K_LTM, no markers, profiler off), the mean over `--calls` calls; the wall time of a call (host clock around calls that end in
a stream synchronisation) stands beside them.
Usage: time_ltm_green_weighted.py [--cases svo:150] [--nz 256] [--eta 1e-3] [--calls 2] [--json FILE] [--out FILE]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["svo:150"])
ap.add_argument("--nz", nargs="+", type=int, default=[256])
ap.add_argument("--eta", type=float, default=1e-3)
ap.add_argument("--calls", type=int, default=2)
ap.add_argument("--json", default=None)
ap.add_argument("--out", default=None, help="also write the printed lines to this file")
args = ap.parse_args()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def make(name):
    if name == "svo":
        return abz.load_w90_series(os.path.join(ROOT, "tests", "golden", "svo_hr.dat.gz"))
    return abz.synthetic_wannier(int(name[3:]), rmax=2, seed=7)


def timed(fn, ctx, calls):
    """(kernel ms, wall ms) of one call: the library's events around the kernels, a host clock around the calls"""
    fn(); ctx.sync()
    t0 = time.perf_counter()
    for _ in range(calls): fn()
    ctx.sync()
    wall = 1e3 * (time.perf_counter() - t0) / calls
    ctx.prof_enable(True, kernels=[L.K_LTM]); ctx.prof_reset()
    for _ in range(calls): fn()
    ctx.sync()
    ms, _ = ctx.prof_read(L.K_LTM); ctx.prof_enable(False)
    return ms / calls, wall


rows = []
for case in args.cases:
    name, npt = case.split(":")
    npt = int(npt)
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    lo, hi = (10.0, 15.0) if name == "svo" else (-2.5, 2.5)
    for nz in args.nz:
        zs = np.linspace(lo, hi, nz) + 1j * args.eta
        row = {"series": name, "bands": n, "npt": npt, "nz": nz, "eta": args.eta}
        row["trace_kernel_ms"], row["trace_ms"] = timed(lambda: rule.ltm_green(zs), ctx, args.calls)
        row["energy_kernel_ms"], row["energy_ms"] = timed(lambda: rule.ltm_green(zs, elements="energy"), ctx, args.calls)
        rule.ltm_orbitals()
        row["all_kernel_ms"], row["all_ms"] = timed(lambda: rule.ltm_green(zs, elements="attached"), ctx, args.calls)
        G = rule.ltm_green(zs, elements="attached")
        t = rule.ltm_green(zs)
        row["max_abs_sum_minus_trace"] = float(np.abs(G.sum(axis=1) - t).max())
        row["single_kernel_ms"], row["single_ms"] = [], []
        for a in range(n):
            rule.ltm_orbitals([a])
            k, w = timed(lambda: rule.ltm_green(zs, elements="attached"), ctx, args.calls)
            row["single_kernel_ms"].append(k); row["single_ms"].append(w)
        singles = float(np.sum(row["single_kernel_ms"]))
        row["ratio_energy_over_trace"] = row["energy_kernel_ms"] / row["trace_kernel_ms"]
        row["ratio_all_over_singles"] = row["all_kernel_ms"] / singles
        per = 1e6 / (float(npt) ** s.d * [1, 2, 6][s.d - 1] * n * nz)
        rows.append(row)
        say(f"green weighted {name} n={n} npt={npt} nz={nz} eta={args.eta:g}, kernel ms (wall ms):  trace {row['trace_kernel_ms']:.3f} "
            f"({row['trace_ms']:.3f})  | energy, 1 component {row['energy_kernel_ms']:.3f} ({row['energy_ms']:.3f})  | {n} orbital weights in "
            f"one call {row['all_kernel_ms']:.3f} ({row['all_ms']:.3f})  | {n} single-component calls "
            + " + ".join(f"{k:.3f}" for k in row["single_kernel_ms"]) + f" = {singles:.3f}")
        say(f"    ns per (simplex, z): trace {per * row['trace_kernel_ms']:.4f}, 1 component {per * row['energy_kernel_ms']:.4f}, {n} components "
            f"{per * row['all_kernel_ms']:.4f}  | weighted(1 component) / trace = {row['ratio_energy_over_trace']:.3f}  | {n}-component call / "
            f"{n} single-component calls = {row['ratio_all_over_singles']:.3f}  | max |sum_a G_aa - tr G| {row['max_abs_sum_minus_trace']:.3e}")
    rule.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

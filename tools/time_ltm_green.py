"""Tetrahedron trace of the Green's function (abz_rule_ltm_green) against the two existing scans over the same grid: the g scan
abz_rule_ltm at the same real energies (eigenvalue rule) and the resolvent scan abz_rule_reduce(ABZ_F_DOS) at the same
z = E + i eta (a rule of H(k) on the same grid).  One session; every call is warmed up first; wall times are host clocks
around calls that end in a stream synchronisation, the median of `--repeats` repeats of `--calls` calls each, profiler off;
the kernel times beside them come from the library's own HIP events (ABZ_K_LTM / ABZ_K_REDUCE) in a separate pass.
Usage: time_ltm_green.py [--cases svo:24 svo:48 svo:150 syn16:24] [--nz 32 256] [--eta 1e-3] [--repeats 3] [--calls 5] [--json FILE] [--out FILE]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["svo:24", "svo:48", "svo:150", "syn16:24"])
ap.add_argument("--nz", nargs="+", type=int, default=[32, 256])
ap.add_argument("--eta", type=float, default=1e-3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--calls", type=int, default=5)
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


def median_ms(fn, ctx, calls):
    """median over the repeats of the mean wall time of a call, ms"""
    fn(); ctx.sync()
    ts = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(calls): fn()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0) / calls)
    return float(np.median(ts))


def kernel_ms(fn, ctx, kid, calls):
    """time of one call's kernels from the library's events, ms"""
    ctx.prof_enable(True, kernels=[kid]); ctx.prof_reset()
    for _ in range(calls): fn()
    ctx.sync()
    ms, _ = ctx.prof_read(kid); ctx.prof_enable(False)
    return ms / calls


rows = []
for case in args.cases:
    name, npt = case.split(":")
    npt = int(npt)
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    re_ = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    rh = abz.DeviceRule(dev, npt, None, L.WANT_H)
    lo, hi = (10.0, 15.0) if name == "svo" else (-2.5, 2.5)
    for nz in args.nz:
        Es = np.linspace(lo, hi, nz)
        zs = Es + 1j * args.eta
        # a call of the trace takes a large multiple of a scan's time on the big grid: fewer calls per repeat there
        calls_g = max(1, args.calls if npt ** s.d * n * nz < 5e8 else 1)
        row = {"series": name, "bands": n, "npt": npt, "nz": nz, "eta": args.eta}
        for key, fn, kid, calls in (("green", lambda: re_.ltm_green(zs), L.K_LTM, calls_g), ("ltm_g", lambda: re_.ltm(Es), L.K_LTM, args.calls),
                                    ("reduce_dos", lambda: rh.reduce(L.F_DOS, [args.eta], Es), L.K_REDUCE, args.calls)):
            row[key + "_ms"] = median_ms(fn, ctx, calls)
            row[key + "_kernel_ms"] = kernel_ms(fn, ctx, kid, calls)
        t = re_.ltm_green(zs)
        g = re_.ltm(Es)
        p = rh.reduce(L.F_DOS, [args.eta], Es)[:, 0].real
        row["max_abs_green_minus_g"] = float(np.abs(-t.imag / np.pi - g).max())
        row["max_abs_reduce_minus_g"] = float(np.abs(p - g).max())
        row["ns_per_simplex_z"] = 1e6 * row["green_kernel_ms"] / (float(npt) ** s.d * [1, 2, 6][s.d - 1] * n * nz)
        rows.append(row)
        say(f"green {name} n={n} npt={npt} nz={nz} eta={args.eta:g}: ltm_green {row['green_ms']:.4f} ms (kernels {row['green_kernel_ms']:.4f}, "
            f"{row['ns_per_simplex_z']:.4f} ns per simplex and z)  | g scan {row['ltm_g_ms']:.4f} ms (kernels {row['ltm_g_kernel_ms']:.4f})  | "
            f"resolvent scan {row['reduce_dos_ms']:.4f} ms (kernels {row['reduce_dos_kernel_ms']:.4f})  | max |-Im trG/pi - g| "
            f"{row['max_abs_green_minus_g']:.3e}, max |resolvent sum - g| {row['max_abs_reduce_minus_g']:.3e}")
    re_.close(); rh.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

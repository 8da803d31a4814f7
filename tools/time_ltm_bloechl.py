"""The curvature-corrected weighted state sum (ABZ_LTM_STATES_CORRECTED of abz_rule_ltm_weighted) against the plain N_A
scan on the same rule, elements and energies, alternating, in one process: A = e ("energy") and attached random elements
of 1 and 3 components.  Profiler off, every variant warmed; wall times are host clocks around calls that end in a stream
synchronisation, the median of `--repeats` repeats of `--calls` calls each; the kernel times beside them come from the
library's own HIP events (ABZ_K_LTM) in a separate pass.  The plain scan is timed right before and right after the
corrected one: the yardstick of that very moment.
Usage: time_ltm_bloechl.py [--cases svo:48 svo:150 syn16:24] [--nE 32 256] [--ncomp 1 3] [--repeats 5] [--calls 20]
                           [--json FILE]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["svo:48", "svo:150", "syn16:24"], help="series:npt")
ap.add_argument("--nE", nargs="+", type=int, default=[32, 256])
ap.add_argument("--ncomp", nargs="+", type=int, default=[1, 3])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
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


def kernel_ms(fn, ctx):
    """(time of a call's kernels from the library's events, ms; profiled launches per call)"""
    ctx.prof_enable(True, kernels=[L.K_LTM]); ctx.prof_reset()
    for _ in range(args.calls): fn()
    ctx.sync()
    ms, n = ctx.prof_read(L.K_LTM); ctx.prof_enable(False)
    return ms / args.calls, n / args.calls


rows = []
for case in args.cases:
    name, npt = case.split(":")
    npt = int(npt)
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    lo, hi = (10.0, 15.0) if name == "svo" else (-2.5, 2.5)
    rng = np.random.default_rng(1)
    for nE in args.nE:
        Es = np.linspace(lo, hi, nE)
        for key, el, ncomp in [("energy", "energy", 1)] + [(f"attached{c}", "attached", c) for c in args.ncomp]:
            if el == "attached":
                rule.ltm_elements(rng.standard_normal((ncomp, rule.nk, n)))
            plain = lambda: rule.ltm(Es, states=True, elements=el)
            corr = lambda: rule.ltm(Es, states=True, elements=el, correction=True)
            p0 = median_ms(plain, ctx)
            med, lo_, hi_ = median_ms(corr, ctx)
            p1 = median_ms(plain, ctx)
            kp, _ = kernel_ms(plain, ctx)
            kc, launches = kernel_ms(corr, ctx)
            row = {"series": name, "bands": n, "npt": npt, "nE": nE, "variant": key, "ncomp": ncomp, "ms": med, "minmax_ms": (lo_, hi_),
                   "plain_before_ms": p0[0], "plain_after_ms": p1[0], "kernel_ms": kc, "plain_kernel_ms": kp, "scopes_per_call": launches}
            rows.append(row)
            print(f"BLOECHL {name} n={n} npt={npt} nE={nE} {key:10s}: corrected {med:.4f} ms [{lo_:.4f}, {hi_:.4f}] | plain before {p0[0]:.4f} "
                  f"after {p1[0]:.4f} ms | kernels corrected {kc:.4f} plain {kp:.4f} ms (x{kc / kp:.3f}, {launches:.0f} scans)", flush=True)
    rule.ltm_elements(None)
    rule.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)

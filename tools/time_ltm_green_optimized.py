"""The Green's functions of the optimized tetrahedron rule (abz_rule_ltm_green_optimized) against the linear ones
(abz_rule_ltm_green, abz_rule_ltm_green_weighted) of the same rule and the same z, alternating, in one process: the trace and
attached random elements of 1 and 4 components.  Times are the kernels' own, from the library's HIP events (ABZ_K_LTM): every
variant is warmed, then `--repeats` rounds time linear, optimized, linear, optimized ... and the medians are reported with the
extremes, so that the linear kernels' times (unchanged object code) stand beside the new one's from the same run.  For grids
given as `--double` the linear call is also timed at 2 npt, the grid whose accuracy the optimized rule matches, together with the
wall time of building each rule (eigen-solves included): the optimized rule at npt is to be judged against the linear rule at
2 npt plus its 8-fold build.
Usage: time_ltm_green_optimized.py [--cases svo:48 svo:150] [--double 48] [--nz 32 256] [--ncomp 1 4] [--eta 1e-2] [--repeats 3]
       [--calls 2] [--out FILE]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["svo:48", "svo:150"], help="series:npt")
ap.add_argument("--double", nargs="*", type=int, default=[48], help="npt whose linear call is also timed at 2 npt")
ap.add_argument("--nz", nargs="+", type=int, default=[32, 256])
ap.add_argument("--ncomp", nargs="+", type=int, default=[1, 4])
ap.add_argument("--eta", type=float, default=1e-2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--calls", type=int, default=2, help="calls per timing (1 from 100^3 on)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ltm_green_optimized_vs_linear.txt"))
args = ap.parse_args()


def make(name):
    if name == "svo":
        return abz.load_w90_series(os.path.join(ROOT, "tests", "golden", "svo_hr.dat.gz"))
    return abz.synthetic_wannier(int(name[3:]), rmax=2, seed=7)


def kernel_ms(fn, ctx, calls):
    """time of a call's kernels from the library's events, ms"""
    ctx.prof_enable(True, kernels=[L.K_LTM]); ctx.prof_reset()
    for _ in range(calls): fn()
    ctx.sync()
    ms, _ = ctx.prof_read(L.K_LTM); ctx.prof_enable(False)
    return ms / calls


def alternate(fns, ctx, calls):
    """fns: label -> call.  Warm each, then `repeats` rounds over all of them in turn -> label -> (median, min, max) ms"""
    for fn in fns.values(): fn()
    ctx.sync()
    ts = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, fn in fns.items(): ts[k].append(kernel_ms(fn, ctx, calls))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def build_ms(dev, npt):
    """(rule, median wall time of building it, ms)"""
    ts, rule = [], None
    for _ in range(args.repeats):
        if rule is not None: rule.close()
        dev.ctx.sync(); t0 = time.perf_counter()
        rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG); rule.h; dev.ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return rule, float(np.median(ts))


lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


fmt = lambda t: f"{t[0]:.3f} ms [{t[1]:.3f}, {t[2]:.3f}]"
for case in args.cases:
    name, npt = case.split(":")
    npt = int(npt)
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    rule, tb = build_ms(dev, npt)
    twice = npt in args.double
    if twice: rule2, tb2 = build_ms(dev, 2 * npt)
    say(f"GOPTLTM {name} n={n} npt={npt}: rule build {tb:.2f} ms" + (f" | npt={2 * npt}: rule build {tb2:.2f} ms" if twice else ""))
    lo, hi = (10.0, 15.0) if name == "svo" else (-2.5, 2.5)
    rng = np.random.default_rng(1)
    calls = 1 if npt >= 100 else args.calls
    for key, el, ncomp in [("trace", None, 1)] + [(f"attached{c}", "attached", c) for c in args.ncomp]:
        if el == "attached":
            rule.ltm_elements(rng.standard_normal((ncomp, rule.nk, n)))
            if twice: rule2.ltm_elements(rng.standard_normal((ncomp, rule2.nk, n)))
        for nz in args.nz:
            zs = np.linspace(lo, hi, nz) + 1j * args.eta
            fns = {"linear": lambda: rule.ltm_green(zs, elements=el), "optimized": lambda: rule.ltm_green_optimized(zs, elements=el)}
            if twice: fns["linear2"] = lambda: rule2.ltm_green(zs, elements=el)
            t = alternate(fns, ctx, calls)
            line = (f"GOPTLTM {name} n={n} npt={npt} nz={nz} {key:9s}: kernels optimized {fmt(t['optimized'])} | linear {fmt(t['linear'])} "
                    f"(x{t['optimized'][0] / t['linear'][0]:.2f})")
            if twice:
                line += (f" | linear at npt={2 * npt} {fmt(t['linear2'])} (optimized x{t['optimized'][0] / t['linear2'][0]:.2f}); with the rule "
                         f"builds: optimized {tb + t['optimized'][0]:.2f} ms, linear at {2 * npt} {tb2 + t['linear2'][0]:.2f} ms "
                         f"(x{(tb + t['optimized'][0]) / (tb2 + t['linear2'][0]):.2f})")
            say(line)
    rule.ltm_elements(None); rule.close()
    if twice: rule2.close()
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")

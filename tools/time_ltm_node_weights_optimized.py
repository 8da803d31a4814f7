"""The integration weights of the optimized tetrahedron rule (abz_rule_ltm_node_weights_optimized) beside what they stand next to,
on the same rule and the same energies, alternating, in one process: the linear weights (abz_rule_ltm_node_weights), the N_A / g_A
scan of abz_rule_ltm_optimized with 4 attached components, and abz_rule_ltm_node_weights_dot on the optimized and on a linear
block.  Times are the kernels' own, from the library's HIP events (ABZ_K_LTM): every variant is warmed, then `--repeats` rounds
time them in turn and the medians are reported with the extremes.

The events of a call span both of its kernels.  The split into kernel A (ltm_opt_cornerw_kernel, the corner weights of a slab)
and kernel B (ltm_opt_nodew_gather_kernel) comes from a kernel trace, in a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_ltm_node_weights_optimized.py --trace --plan DIR/plan.json
    python tools/time_ltm_node_weights_optimized.py --from-trace DIR --plan DIR/plan.json
The first makes, per case, one warming call and `--calls` timed calls in a fixed order and writes that order down; the second cuts
the trace's dispatches of the two kernels along it and appends the per-call sums to the output file.
Usage: time_ltm_node_weights_optimized.py [--cases svo:48 svo:150] [--nE 1 4 16] [--repeats 3] [--calls 2] [--caps 64 256 1024 8192] [--out FILE]"""
import argparse, csv, glob, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["svo:48", "svo:150"], help="series:npt")
ap.add_argument("--nE", nargs="+", type=int, default=[1, 4, 16])
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--calls", type=int, default=2, help="calls per timing (1 from 100^3 on)")
ap.add_argument("--caps", nargs="*", type=int, default=[64, 256, 1024, 8192], help="values of ABZ_LTM_OPTW_CHUNK_MB (MB) the weights are also timed under")
ap.add_argument("--trace", action="store_true", help="the fixed sequence of calls for a kernel trace; needs --plan")
ap.add_argument("--from-trace", default=None, help="directory of a rocprofv3 kernel trace of a --trace run")
ap.add_argument("--plan", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ltm_node_weights_optimized.txt"))
args = ap.parse_args()

KERNEL_A, KERNEL_B = "ltm_opt_cornerw_kernel", "ltm_opt_nodew_gather_kernel"


def launches(n, npt, nE):
    """launches of kernel A (= of kernel B) of one call: groups of 4 energies, then single ones, each over its slabs of grid planes
    (the arithmetic of launch_ltm_node_weights_optimized, with the cap of ABZ_LTM_OPTW_CHUNK_MB as the library reads it)"""
    env = os.environ.get("ABZ_LTM_OPTW_CHUNK_MB", "")
    cap_mb = int(env) if env.strip() and int(env) > 0 else 256

    def slabs(ne):
        fit = (cap_mb << 20) // (8 * 24 * n * ne * npt * npt)
        S = min(npt, max(1, fit - 3))
        return 1 if S + 3 >= npt else -(-npt // S)
    return (nE // 4) * slabs(4) + (nE % 4 if nE >= 4 else nE) * slabs(1)


if args.from_trace:
    plan = json.load(open(args.plan))
    files = glob.glob(os.path.join(args.from_trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = [r for r in csv.DictReader(open(files[0])) if KERNEL_A in r["Kernel_Name"] or KERNEL_B in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = {k: [1e-6 * (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows if k in r["Kernel_Name"]] for k in (KERNEL_A, KERNEL_B)}
    assert len(ms[KERNEL_A]) == len(ms[KERNEL_B]) == sum(p["launches"] * (1 + p["calls"]) for p in plan), (len(ms[KERNEL_A]), len(ms[KERNEL_B]))
    at, lines = 0, []
    for p in plan:
        at += p["launches"]  # the warming call
        a = [sum(ms[KERNEL_A][at + c * p["launches"]: at + (c + 1) * p["launches"]]) for c in range(p["calls"])]
        b = [sum(ms[KERNEL_B][at + c * p["launches"]: at + (c + 1) * p["launches"]]) for c in range(p["calls"])]
        at += p["calls"] * p["launches"]
        lines.append(f"OPTW-TRACE {p['label']}: {p['launches']} launches of each kernel per call | kernel A {np.median(a):.3f} ms "
                     f"[{min(a):.3f}, {max(a):.3f}] | kernel B {np.median(b):.3f} ms [{min(b):.3f}, {max(b):.3f}] | B / A x{np.median(b) / np.median(a):.2f}")
    print("\n".join(lines))
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0)

import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L


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


lines, plan = [], []


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
    rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    lo, hi = (10.0, 15.0) if name == "svo" else (-2.5, 2.5)
    calls = 1 if npt >= 100 else args.calls
    if not args.trace:
        rule.ltm_elements(np.random.default_rng(1).standard_normal((4, rule.nk, n)))
    for nE in args.nE:
        Es = np.linspace(lo, hi, nE + 2)[1:-1]
        for what, states in (("dos", False), ("states", True)):
            label = f"{name} n={n} npt={npt} nE={nE} {what}"
            opt = lambda: rule.ltm_node_weights_optimized(Es, states=states, export=False)
            if args.trace:
                for _ in range(1 + calls): opt()
                ctx.sync()
                plan.append(dict(label=label, launches=launches(n, npt, nE), calls=calls))  # (the cap of THIS run: --from-trace reads the plan, not the environment)
                continue
            lin = lambda: rule.ltm_node_weights(Es, states=states, export=False)
            t = alternate({"optimized": opt, "linear": lin, "scan4": lambda: rule.ltm_optimized(Es, states=states, elements="attached")}, ctx, calls)
            # the dot reads whichever block is resident: 4 components against nE sets
            opt(); d_opt = alternate({"dot": lambda: rule.ltm_node_weights_dot()}, ctx, calls)["dot"]
            lin(); d_lin = alternate({"dot": lambda: rule.ltm_node_weights_dot()}, ctx, calls)["dot"]
            say(f"OPTW {label}: kernels A + B {fmt(t['optimized'])} in {launches(n, npt, nE)} launches each | linear weights {fmt(t['linear'])} "
                f"(x{t['optimized'][0] / t['linear'][0]:.2f}) | ltm_optimized scan, 4 components {fmt(t['scan4'])} "
                f"(weights x{t['optimized'][0] / t['scan4'][0]:.2f}) | dot of 4 components on the optimized block {fmt(d_opt)}, on a linear block {fmt(d_lin)}")
    if not args.trace and args.caps:
        # the cap on the corner weights' scratch: the same bits, other slab heights (4 and 16 energies, ABZ_LTM_STATES)
        before = os.environ.get("ABZ_LTM_OPTW_CHUNK_MB")
        for nE in (4, 16):
            Es = np.linspace(lo, hi, nE + 2)[1:-1]
            parts = []
            for cap in args.caps:
                os.environ["ABZ_LTM_OPTW_CHUNK_MB"] = str(cap)
                t = alternate({"optimized": lambda: rule.ltm_node_weights_optimized(Es, export=False)}, ctx, calls)["optimized"]
                parts.append(f"{cap} MB: {launches(n, npt, nE)} launches, {fmt(t)}")
            say(f"OPTW-CAP {name} n={n} npt={npt} nE={nE} states: kernels A + B under ABZ_LTM_OPTW_CHUNK_MB = " + " | ".join(parts))
        if before is None: os.environ.pop("ABZ_LTM_OPTW_CHUNK_MB")
        else: os.environ["ABZ_LTM_OPTW_CHUNK_MB"] = before
    rule.ltm_elements(None); rule.close()
if args.trace:
    json.dump(plan, open(args.plan, "w"), indent=1)
else:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

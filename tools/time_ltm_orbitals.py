"""Orbital weights |U_ab(k)|^2 as LTM matrix elements: the device route (abz_rule_ltm_orbitals) against the host route
(export H, numpy.linalg.eigh, abz_rule_ltm_elements), on the same grid in one process.  The device route is timed twice: on a
rule of eigenvalues only (the call builds a transient H rule, runs the weight kernel and destroys the rule) and on a rule
that holds H (the weight kernel alone).  Wall times are host clocks around calls that end in a stream synchronisation, the
median of `--repeats` repeats; the split beside them comes from the library's own HIP events in a separate pass: ABZ_K_CONTRACT
+ ABZ_K_EVAL are the transient build, ABZ_K_EIG the weight kernel.  The host route runs `--host-repeats` times (one at 150^3:
3.4 M LAPACK calls).  One scan of the attached weights is timed beside them for scale.  No speed-up is asserted.
Usage: time_ltm_orbitals.py [--cases svo:48 svo:150 syn16:24] [--repeats 5] [--host-repeats 1] [--no-host] [--json FILE]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["svo:48", "svo:150", "syn16:24"])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--host-repeats", type=int, default=1)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()


def make(name):
    if name == "svo":
        return abz.load_w90_series(os.path.join(ROOT, "tests", "golden", "svo_hr.dat.gz"))
    return abz.synthetic_wannier(int(name[3:]), rmax=2, seed=7)


def median_ms(fn, ctx, repeats):
    fn(); ctx.sync()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def event_ms(fn, ctx, repeats):
    """per call: {slot: (ms of its kernels from the library's events, profiled scopes)}"""
    slots = {"contract": L.K_CONTRACT, "eval": L.K_EVAL, "eig": L.K_EIG}
    ctx.prof_enable(True, kernels=list(slots.values())); ctx.prof_reset()
    for _ in range(repeats): fn()
    ctx.sync()
    out = {k: tuple(v / repeats for v in ctx.prof_read(i)) for k, i in slots.items()}
    ctx.prof_enable(False)
    return out


def host_route(rule_h):
    ex = rule_h.export(x=False, w=False, H=True)
    _, U = np.linalg.eigh(ex["H"])
    rule_h.ltm_elements(np.ascontiguousarray((np.abs(U) ** 2).transpose(1, 0, 2)))


rows = []
for case in args.cases:
    name, npt = case.split(":")
    npt = int(npt)
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    rule_e = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    rule_h = abz.DeviceRule(dev, npt, None, L.WANT_H | L.WANT_EIG)
    lo, hi = (10.0, 15.0) if name == "svo" else (-2.5, 2.5)
    Es = np.linspace(lo, hi, 256)
    row = {"series": name, "bands": n, "npt": npt, "nodes": npt ** 3}
    for key, rule in (("device_transient", rule_e), ("device_resident_H", rule_h)):
        fn = lambda: rule.ltm_orbitals()
        med, lo_, hi_ = median_ms(fn, ctx, args.repeats)
        ev = event_ms(fn, ctx, args.repeats)
        row[key] = {"ms": med, "minmax_ms": (lo_, hi_), "build_kernels_ms": ev["contract"][0] + ev["eval"][0], "weight_kernel_ms": ev["eig"][0],
                    "scopes": {k: v[1] for k, v in ev.items()}}
        print(f"ORB {name} n={n} npt={npt} {key:18s}: {med:.3f} ms [{lo_:.3f}, {hi_:.3f}]  kernels: build {row[key]['build_kernels_ms']:.3f} + "
              f"weights {row[key]['weight_kernel_ms']:.3f} ms", flush=True)
    scan = median_ms(lambda: rule_e.ltm(Es, elements="attached"), ctx, args.repeats)
    row["scan_256E_ms"] = scan[0]
    print(f"ORB {name} n={n} npt={npt} scan of the weights, 256 energies: {scan[0]:.3f} ms", flush=True)
    if not args.no_host:
        med, lo_, hi_ = median_ms(lambda: host_route(rule_h), ctx, args.host_repeats)
        row["host"] = {"ms": med, "minmax_ms": (lo_, hi_)}
        print(f"ORB {name} n={n} npt={npt} host (export + eigh + attach): {med:.1f} ms [{lo_:.1f}, {hi_:.1f}]", flush=True)
    rows.append(row)
    rule_e.close(); rule_h.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)

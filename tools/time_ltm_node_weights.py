"""Integration weights per node (abz_rule_ltm_node_weights), their export, dot (abz_rule_ltm_node_weights_dot) and fold
(abz_rule_ltm_node_weights_fold) against the weighted scan ltm(Es, states=True, elements="energy") of the same rule and energies,
alternating, in one process: 1 and 16 energies, ABZ_LTM_STATES and ABZ_LTM_STATES_CORRECTED.  Profiler off, every variant warmed;
wall times are host clocks around calls that end in a stream synchronisation, the median of `--repeats` repeats of `--calls` calls
each; the kernel times beside them come from the library's own HIP events (ABZ_K_LTM) in a separate pass.  The dot reports the
bytes it reads (the weight block once, the element block once per energy) over its kernel time.
Usage: time_ltm_node_weights.py [--series svo syn16] [--npt 24 48] [--nE 1 16] [--ncomp 16] [--fold-npt 48]
                                [--repeats 5] [--calls 10] [--json FILE]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--series", nargs="+", default=["svo"])
ap.add_argument("--npt", nargs="+", type=int, default=[24, 48])
ap.add_argument("--nE", nargs="+", type=int, default=[1, 16])
ap.add_argument("--ncomp", type=int, default=16)
ap.add_argument("--fold-npt", nargs="*", type=int, default=[])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--json", default=None)
args = ap.parse_args()


def make(name):
    if name == "svo":
        return abz.load_w90_series(os.path.join(ROOT, "tests", "golden", "svo_hr.dat.gz"))
    return abz.synthetic_wannier(int(name[3:]), rmax=2, seed=7)


def median_ms(fn, ctx, calls=None):
    """median over the repeats of the mean wall time of a call, ms"""
    calls = calls or args.calls
    fn(); ctx.sync()
    ts = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(calls): fn()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0) / calls)
    return float(np.median(ts))


def kernel_ms(fn, ctx, calls=None):
    """time of a call's kernels from the library's events, ms"""
    calls = calls or args.calls
    fn(); ctx.sync()
    ctx.prof_enable(True, kernels=[L.K_LTM]); ctx.prof_reset()
    for _ in range(calls): fn()
    ctx.sync()
    ms, _ = ctx.prof_read(L.K_LTM); ctx.prof_enable(False)
    return ms / calls


rows = []
for name in args.series:
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    for npt in sorted(set(args.npt) | set(args.fold_npt)):
        rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
        lo, hi = (11.0, 14.0) if name == "svo" else (-2.0, 2.0)
        row_len = (npt + 15) // 16 * 16
        rule.ltm_elements(np.random.default_rng(1).standard_normal((args.ncomp, rule.nk, n)))
        for nE in args.nE:
            Es = np.linspace(lo, hi, nE + 2)[1:-1]
            for correction in (False, True):
                what = "STATES_CORRECTED" if correction else "STATES"
                scan = lambda: rule.ltm(Es, states=True, elements="energy", correction=correction)
                one = lambda: rule.ltm(Es[:1], states=True, elements="energy", correction=correction)
                weights = lambda: rule.ltm_node_weights(Es, correction=correction, export=False)
                export = lambda: rule.ltm_node_weights(Es, correction=correction)
                dot = lambda: rule.ltm_node_weights_dot()
                # the shipped scan right before and right after: the yardstick of this very moment
                s0 = median_ms(scan, ctx)
                w_ms, x_ms = median_ms(weights, ctx), median_ms(export, ctx, calls=max(1, args.calls // 5))
                weights()
                d_ms = median_ms(dot, ctx)
                s1 = median_ms(scan, ctx)
                k_scan, k_one, k_w = kernel_ms(scan, ctx), kernel_ms(one, ctx), kernel_ms(weights, ctx)
                weights()
                k_dot = kernel_ms(dot, ctx)
                read = 8.0 * npt ** 2 * n * row_len * (nE + nE * args.ncomp)  # the weights once, the elements once per energy
                row = {"series": name, "bands": n, "npt": npt, "nE": nE, "what": what, "ncomp": args.ncomp,
                       "weights_ms": w_ms, "weights_kernel_ms": k_w, "export_ms": x_ms, "dot_ms": d_ms, "dot_kernel_ms": k_dot,
                       "dot_read_GBps": read / (k_dot * 1e-3) / 1e9, "scan_before_ms": s0, "scan_after_ms": s1, "scan_kernel_ms": k_scan,
                       "scan_one_energy_kernel_ms": k_one, "ratio_to_one_energy_scan": k_w / k_one}
                rows.append(row)
                print(f"NODEW {name} n={n} npt={npt} nE={nE} {what:16s}: weights {w_ms:.4f} ms (kernels {k_w:.4f}), with export {x_ms:.3f} ms, "
                      f"dot x{args.ncomp} {d_ms:.4f} ms (kernels {k_dot:.4f}, {row['dot_read_GBps']:.0f} GB/s read)  | scan(energy) before "
                      f"{s0:.4f} after {s1:.4f} ms (kernels {k_scan:.4f}; one energy {k_one:.4f}: weights / that = {k_w / k_one:.2f})", flush=True)
        rule.close()
        if npt in args.fold_npt and s.d == 3:
            bz = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
            unf = abz.DeviceRule(dev, npt, bz.syms, L.WANT_EIG).unfold()
            for nE in args.nE:
                Es = np.linspace(lo, hi, nE + 2)[1:-1]
                unf.ltm_node_weights(Es, export=False)
                unf.ltm_node_weights_fold()  # (the inverse of the orbit map is made here, once)
                f_ms, k_f = median_ms(unf.ltm_node_weights_fold, ctx), kernel_ms(unf.ltm_node_weights_fold, ctx)
                rows.append({"series": name, "bands": n, "npt": npt, "nE": nE, "variant": "fold", "nirr": unf.source.nk, "fold_ms": f_ms,
                             "fold_kernel_ms": k_f})
                print(f"NODEW {name} n={n} npt={npt} nE={nE} fold onto {unf.source.nk} nodes: {f_ms:.4f} ms (kernel {k_f:.4f})", flush=True)
            unf.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)

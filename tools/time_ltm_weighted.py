"""Weighted tetrahedron scans (abz_rule_ltm_weighted) and the Fermi search (abz_rule_ltm_fermi) against the unweighted
abz_rule_ltm on the same rule and energies, alternating, in one process: A = e ("energy") and attached random elements
of 1, 3 and 16 components, for g_A(E) and N_A(E); the Fermi level against a host bisection of abz_rule_ltm(STATES) to
the same width.  Profiler off, every variant warmed; wall times are host clocks around calls that end in a stream
synchronisation, the median of `--repeats` repeats of `--calls` calls each; the kernel times beside them come from the
library's own HIP events (ABZ_K_LTM) in a separate pass.
Usage: time_ltm_weighted.py [--series svo syn16] [--npt 24 48] [--nE 32 256] [--ncomp 1 3 16] [--fermi-npt 150]
                            [--repeats 5] [--calls 20] [--json FILE]"""
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
ap.add_argument("--ncomp", nargs="+", type=int, default=[1, 3, 16])
ap.add_argument("--fermi-npt", nargs="*", type=int, default=[])
ap.add_argument("--fermi-tol", type=float, default=1e-10)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernel_ms(fn, ctx, calls=None):
    """(time of a call's kernels from the library's events, ms; profiled launches per call)"""
    calls = calls or args.calls
    ctx.prof_enable(True, kernels=[L.K_LTM]); ctx.prof_reset()
    for _ in range(calls): fn()
    ctx.sync()
    ms, n = ctx.prof_read(L.K_LTM); ctx.prof_enable(False)
    return ms / calls, n / calls


def host_bisection(rule, nstates, tol):
    """The Fermi level without abz_rule_ltm_fermi: bisect N(E) from the host, one synchronising call per step."""
    eig = rule.export(x=False, w=False, eig=True)["eig"]
    lo, hi = float(eig.min()), float(eig.max())

    def run():
        a, b = lo, hi
        steps = 0
        while b - a > tol:
            m = 0.5 * (a + b)
            if not (a < m < b):
                break
            if rule.ltm(np.array([m]), states=True)[0] >= nstates * (1 - 1e-12):
                b = m
            else:
                a = m
            steps += 1
        return b, steps
    return run


rows = []
for name in args.series:
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    for npt in sorted(set(args.npt) | set(args.fermi_npt)):
        rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
        lo, hi = (10.0, 15.0) if name == "svo" else (-2.5, 2.5)
        rng = np.random.default_rng(1)
        if npt in args.npt:
            for nE in args.nE:
                Es = np.linspace(lo, hi, nE)
                variants = [("plain", None, 0), ("energy", "energy", 1)] + [(f"attached{c}", "attached", c) for c in args.ncomp]
                for states in (False, True):
                    for key, el, ncomp in variants:
                        if el == "attached":
                            rule.ltm_elements(rng.standard_normal((ncomp, rule.nk, n)))
                        fn = lambda: rule.ltm(Es, states=states, elements=el)
                        base = lambda: rule.ltm(Es, states=states)
                        # the shipped scan right before and right after every variant: the yardstick of this very moment
                        b0 = median_ms(base, ctx)
                        med, lo_, hi_ = median_ms(fn, ctx)
                        b1 = median_ms(base, ctx)
                        kms, launches = kernel_ms(fn, ctx)
                        row = {"series": name, "bands": n, "npt": npt, "nE": nE, "what": "N" if states else "g", "variant": key, "ncomp": ncomp,
                               "ms": med, "minmax_ms": (lo_, hi_), "kernel_ms": kms, "scopes_per_call": launches,
                               "plain_before_ms": b0[0], "plain_after_ms": b1[0]}
                        rows.append(row)
                        print(f"WLTM {name} n={n} npt={npt} nE={nE} {row['what']} {key:11s}: {med:.4f} ms [{lo_:.4f}, {hi_:.4f}] (kernels {kms:.4f}, "
                              f"{launches:.0f} scans)  | plain before {b0[0]:.4f} after {b1[0]:.4f} ms", flush=True)
                rule.ltm_elements(None)
        if npt in args.fermi_npt:
            nstates = 1.0 if n == 3 else 0.5 * n
            tol = args.fermi_tol
            fermi = lambda: rule.ltm_fermi(nstates, tol)
            bis = host_bisection(rule, nstates, tol)
            f_ms = median_ms(fermi, ctx, calls=5)
            b_ms = median_ms(bis, ctx, calls=2)
            kms, launches = kernel_ms(fermi, ctx, calls=5)
            ef, nf = fermi()
            eb, steps = bis()
            row = {"series": name, "bands": n, "npt": npt, "variant": "fermi", "nstates": nstates, "tol": tol, "ms": f_ms[0], "minmax_ms": f_ms[1:],
                   "kernel_ms": kms, "scopes_per_call": launches, "bisection_ms": b_ms[0], "bisection_steps": steps, "E_F": ef, "N_F": nf,
                   "E_F_bisection": eb}
            rows.append(row)
            print(f"FERMI {name} n={n} npt={npt} nstates={nstates} tol={tol:g}: {f_ms[0]:.4f} ms [{f_ms[1]:.4f}, {f_ms[2]:.4f}] (kernels {kms:.4f}, "
                  f"{launches - 1:.0f} scans + 1 bracket)  | host bisection {b_ms[0]:.4f} ms, {steps} steps  | E_F {ef:.12f} vs {eb:.12f}, "
                  f"N(E_F) - nstates = {nf - nstates:.3e}", flush=True)
        rule.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)

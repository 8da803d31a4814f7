"""The optimized tetrahedron scan (abz_rule_ltm_optimized) against the plain scan (abz_rule_ltm) and the weighted scan
(abz_rule_ltm_weighted) of the same rule and energies, alternating, in one process: g and N with A = 1, A = e ("energy") and
attached random elements of 1 and 4 components.  Profiler off, every variant warmed; wall times are host clocks around calls
that end in a stream synchronisation, the median of `--repeats` repeats of `--calls` calls each; the kernel times beside them come
from the library's own HIP events (ABZ_K_LTM) in a separate pass.  The linear scan is timed right before and right after the
optimized one: the yardstick of that very moment.  The last column counts what the optimized kernel asks for per call -- 8-byte
loads (20 per simplex, band and component, plus 20 more per simplex and band for the energies under attached elements) and FMAs of
the product (68 per simplex and product) -- so that the time can be set against load and VALU rates.
Usage: time_ltm_optimized.py [--cases svo:48 svo:150] [--nE 32 256] [--ncomp 1 4] [--repeats 5] [--calls 10] [--out FILE]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["svo:48", "svo:150"], help="series:npt")
ap.add_argument("--nE", nargs="+", type=int, default=[32, 256])
ap.add_argument("--ncomp", nargs="+", type=int, default=[1, 4])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ltm_optimized_vs_plain.txt"))
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
    """time of a call's kernels from the library's events, ms"""
    ctx.prof_enable(True, kernels=[L.K_LTM]); ctx.prof_reset()
    for _ in range(args.calls): fn()
    ctx.sync()
    ms, _ = ctx.prof_read(L.K_LTM); ctx.prof_enable(False)
    return ms / args.calls


lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


for case in args.cases:
    name, npt = case.split(":")
    npt = int(npt)
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    lo, hi = (10.0, 15.0) if name == "svo" else (-2.5, 2.5)
    rng = np.random.default_rng(1)
    simplices = 6 * npt ** 3 * n
    for nE in args.nE:
        Es = np.linspace(lo, hi, nE)
        for key, el, ncomp in [("one", None, 1), ("energy", "energy", 1)] + [(f"attached{c}", "attached", c) for c in args.ncomp]:
            if el == "attached":
                rule.ltm_elements(rng.standard_normal((ncomp, rule.nk, n)))
            for states in (False, True):
                lin = lambda: rule.ltm(Es, states=states, elements=el)
                opt = lambda: rule.ltm_optimized(Es, states=states, elements=el)
                p0 = median_ms(lin, ctx)
                med, lo_, hi_ = median_ms(opt, ctx)
                p1 = median_ms(lin, ctx)
                kl, ko = kernel_ms(lin, ctx), kernel_ms(opt, ctx)
                groups = 1 if el != "attached" else ncomp // 4 + ((ncomp % 4) >> 1) + (ncomp & 1)  # launches: each loads the energies' stencil
                loads = simplices * 20 * (groups + (ncomp if el == "attached" else 0))
                fmas = simplices * 68 * (groups + (ncomp if el == "attached" else 0))
                say(f"OPTLTM {name} n={n} npt={npt} nE={nE} {key:9s} {'N' if states else 'g'}: optimized {med:.4f} ms [{lo_:.4f}, {hi_:.4f}] | "
                    f"{'plain' if el is None else 'weighted'} before {p0[0]:.4f} after {p1[0]:.4f} ms | kernels optimized {ko:.4f} linear {kl:.4f} ms "
                    f"(x{ko / kl:.2f}) | at most {loads / 1e6:.1f} M loads of 8 B, {fmas / 1e6:.1f} M product FMAs per call: "
                    f"{8e-6 * loads / ko:.0f} GB/s from the caches, {2e-6 * fmas / ko:.0f} GFLOP/s of the product")
    rule.ltm_elements(None)
    rule.close()
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")

"""The complex integration weights W_b(k; z) of the optimized tetrahedron rule (abz_rule_ltm_green_node_weights_optimized)
beside the routes they stand next to, on the same rule, in one process, the routes alternated inside every round:
  new      ltm_green_node_weights_optimized(zs, export=False): corner-weight kernel A' + gather kernel B per group and slab
  linear   ltm_green_node_weights(zs, export=False): the gather of the linear rule
  scan1    ltm_green_optimized(zs, elements="energy"): the optimized scan with one component
  dot4     ltm_green_node_weights_dot() of the resident optimized weights with 4 attached components
  scan4    ltm_green_optimized(zs, elements="attached") with the same 4 components
  matlin   ltm_green_node_weights_matrix(zs): G_pq(z) by the linear rule (gathers included)
  matopt   ltm_green_node_weights_matrix(zs, optimized=True): G_pq(z) by the optimized rule
Per route the median [min, max] over `--rounds` rounds (at least 3) of the wall time of a call (host clock around a call that ends in a
stream synchronisation) and of its kernel times from the library's own HIP events (ABZ_K_LTM; ABZ_K_EIG for the matrix routes).
The values of z per group (NZ) are a constant of the build and the cap of the workspace is the switch ABZ_LTM_OPTW_CHUNK_MB: run
the tool once per build and cap and give `--label` to tell the runs apart.  A' and B separately: run the tool with `--routes new
--rounds 3` under a kernel trace of its own and read the two kernels' rows there.
Usage: time_ltm_green_node_weights_optimized.py [--grids svo:48 svo:150] [--nz 1 8] [--routes new linear ...] [--rounds 3]
                                                [--label TEXT] [--out FILE]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ROUTES = ["new", "linear", "scan1", "dot4", "scan4", "matlin", "matopt"]
ap = argparse.ArgumentParser()
ap.add_argument("--grids", nargs="*", default=["svo:48", "svo:150"])
ap.add_argument("--nz", nargs="+", type=int, default=[1, 8])
ap.add_argument("--routes", nargs="+", default=ROUTES, choices=ROUTES)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--label", default="")
ap.add_argument("--out", default=None)
args = ap.parse_args()
args.rounds = max(3, args.rounds)
lines = []


def say(line):
    lines.append(line)
    print(line, flush=True)


def make(name):
    if name == "svo":
        return abz.load_w90_series(os.path.join(ROOT, "tests", "golden", "svo_hr.dat.gz"))
    return abz.synthetic_wannier(int(name[3:]), rmax=2, seed=7)


def z_values(eig, nz):
    """nz values across the bands at Im z = 1e-2 (one: the middle of the spectrum)"""
    lo, hi = float(eig.min()), float(eig.max())
    return (np.array([0.5 * (lo + hi)]) if nz == 1 else np.linspace(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), nz)) + 1e-2j


def one_call(fn, ctx):
    """(wall, ABZ_K_LTM, ABZ_K_EIG) of one call, ms"""
    ctx.prof_enable(True, kernels=[L.K_EIG, L.K_LTM]); ctx.prof_reset()
    ctx.sync()
    t0 = time.perf_counter(); fn(); ctx.sync()
    wall = 1e3 * (time.perf_counter() - t0)
    ltm, eig = ctx.prof_read(L.K_LTM)[0], ctx.prof_read(L.K_EIG)[0]
    ctx.prof_enable(False)
    return wall, ltm, eig


def med(v):
    return f"{np.median(v):.3f} [{np.min(v):.3f}, {np.max(v):.3f}]"


say(f"# {args.label}  ABZ_LTM_OPTW_CHUNK_MB={os.environ.get('ABZ_LTM_OPTW_CHUNK_MB', '(unset: 256)')}  rounds={args.rounds}")
for case in args.grids:
    name, npt = case.split(":")
    s = make(name); dev = s.device(); ctx = dev.ctx
    need_h = any(r.startswith("mat") for r in args.routes)
    rule = abz.DeviceRule(dev, int(npt), None, (L.WANT_H | L.WANT_H_COMPACT if need_h else 0) | L.WANT_EIG)
    eig = rule.export(x=False, w=False, eig=True)["eig"]
    for nz in args.nz:
        zs = z_values(eig, nz)
        if any(r in args.routes for r in ("dot4", "scan4")):
            rule.ltm_elements(np.random.default_rng(1).standard_normal((4, rule.nk, s.n)))

        def dot4():
            return rule.ltm_green_node_weights_dot()

        fns = {"new": lambda: rule.ltm_green_node_weights_optimized(zs, export=False),
               "linear": lambda: rule.ltm_green_node_weights(zs, export=False),
               "scan1": lambda: rule.ltm_green_optimized(zs, elements="energy"),
               "dot4": dot4,
               "scan4": lambda: rule.ltm_green_optimized(zs, elements="attached"),
               "matlin": lambda: rule.ltm_green_node_weights_matrix(zs),
               "matopt": lambda: rule.ltm_green_node_weights_matrix(zs, optimized=True)}
        got = {r: [] for r in args.routes}
        for rnd in range(args.rounds + 1):  # round 0 warms every route and is not counted
            for r in args.routes:
                if r == "dot4":  # (the resident block must be the optimized one of these zs)
                    rule.ltm_green_node_weights_optimized(zs, export=False)
                t = one_call(fns[r], ctx)
                if rnd:
                    got[r].append(t)
        if "dot4" in args.routes and "scan4" in args.routes:
            rule.ltm_green_node_weights_optimized(zs, export=False)
            d = float(np.abs(dot4() - fns["scan4"]()).max())
            say(f"CHECK {name} npt={npt} nz={nz}: max |dot4 - scan4| = {d:.2e}")
        for r in args.routes:
            w, k, e = (np.array([t[i] for t in got[r]]) for i in range(3))
            say(f"{r:7s} {name} n={s.n} npt={npt} nz={nz}: wall {med(w)} ms  | ABZ_K_LTM {med(k)} ms (per z {np.median(k) / nz:.3f})"
                + (f"  | ABZ_K_EIG {med(e)} ms" if r.startswith("mat") else ""))
        rule.ltm_elements(None)
    rule.close()

if args.out:
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")

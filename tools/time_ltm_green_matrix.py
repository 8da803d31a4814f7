"""Local Green's function matrix of the tetrahedron method (abz_rule_ltm_projectors + abz_rule_ltm_green_weighted) against its
parts on the same eigenvalue rule: the projector attach (all n^2 components of an n <= 4 band series, one group) against the
orbital-weight attach (n components) -- both repeat the eigen-solve of the grid, the transient H build included -- and the
n^2-component Green's call against the n-component diagonal call and the trace, at the same values of z.  One session; every call
is warmed up first; kernel times are the library's own, from its HIP events (ABZ_K_EIG for the attaches, ABZ_K_LTM for the scans,
no markers, profiler off), the mean over `--calls` calls; the wall time of a call (host clock around calls that end in a stream
synchronisation) stands beside them.
Usage: time_ltm_green_matrix.py [--cases svo:150] [--nz 256] [--eta 1e-3] [--calls 2] [--json FILE] [--out FILE]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["svo:150"])
ap.add_argument("--nz", type=int, default=256)
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


def timed(fn, ctx, calls, kernel):
    """(kernel ms, wall ms) of one call: the library's events around the kernels, a host clock around the calls"""
    fn(); ctx.sync()
    t0 = time.perf_counter()
    for _ in range(calls): fn()
    ctx.sync()
    wall = 1e3 * (time.perf_counter() - t0) / calls
    ctx.prof_enable(True, kernels=[kernel]); ctx.prof_reset()
    for _ in range(calls): fn()
    ctx.sync()
    ms, _ = ctx.prof_read(kernel); ctx.prof_enable(False)
    return ms / calls, wall


rows = []
for case in args.cases:
    name, npt = case.split(":")
    npt = int(npt)
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    if n > 4:
        sys.exit(f"{case}: {n} bands are more than one group of projectors (n^2 <= 16 components)")
    rule = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    lo, hi = (10.0, 15.0) if name == "svo" else (-2.5, 2.5)
    zs = np.linspace(lo, hi, args.nz) + 1j * args.eta
    pairs = [(a, a) for a in range(n)] + [(a, b) for a in range(n) for b in range(a + 1, n)]
    row = {"series": name, "bands": n, "npt": npt, "nz": args.nz, "eta": args.eta, "components": n * n}
    row["trace_kernel_ms"], row["trace_ms"] = timed(lambda: rule.ltm_green(zs), ctx, args.calls, L.K_LTM)
    row["orbitals_attach_kernel_ms"], row["orbitals_attach_ms"] = timed(lambda: rule.ltm_orbitals(), ctx, args.calls, L.K_EIG)
    row["diagonal_kernel_ms"], row["diagonal_ms"] = timed(lambda: rule.ltm_green(zs, elements="attached"), ctx, args.calls, L.K_LTM)
    row["projectors_attach_kernel_ms"], row["projectors_attach_ms"] = timed(lambda: rule.ltm_projectors(pairs), ctx, args.calls, L.K_EIG)
    row["matrix_kernel_ms"], row["matrix_ms"] = timed(lambda: rule.ltm_green(zs, elements="attached"), ctx, args.calls, L.K_LTM)
    _, row["green_matrix_ms"] = timed(lambda: rule.ltm_green_matrix(zs), ctx, args.calls, L.K_LTM)
    G = rule.ltm_green_matrix(zs)
    row["max_abs_trace_minus_trace"] = float(np.abs(np.trace(G, axis1=1, axis2=2) - rule.ltm_green(zs)).max())
    row["max_abs_offdiagonal"] = float(np.abs(G - np.einsum("zpp->zp", G)[:, :, None] * np.eye(n)).max())
    rows.append(row)
    say(f"green matrix {name} n={n} npt={npt} nz={args.nz} eta={args.eta:g}, kernel ms (wall ms):  attach {n} orbital weights "
        f"{row['orbitals_attach_kernel_ms']:.3f} ({row['orbitals_attach_ms']:.3f})  | attach {n * n} projector components "
        f"{row['projectors_attach_kernel_ms']:.3f} ({row['projectors_attach_ms']:.3f})  | trace {row['trace_kernel_ms']:.3f} "
        f"({row['trace_ms']:.3f})  | diagonal, {n} components {row['diagonal_kernel_ms']:.3f} ({row['diagonal_ms']:.3f})  | matrix, "
        f"{n * n} components {row['matrix_kernel_ms']:.3f} ({row['matrix_ms']:.3f})  | ltm_green_matrix, attach + scan, wall "
        f"{row['green_matrix_ms']:.3f}")
    say(f"    projector attach / orbital attach = {row['projectors_attach_kernel_ms'] / row['orbitals_attach_kernel_ms']:.3f}  | "
        f"matrix / diagonal = {row['matrix_kernel_ms'] / row['diagonal_kernel_ms']:.3f}  | matrix / trace = "
        f"{row['matrix_kernel_ms'] / row['trace_kernel_ms']:.3f}  | max |sum_p G_pp - tr G| {row['max_abs_trace_minus_trace']:.3e}  | "
        f"max |G_pq|, p != q: {row['max_abs_offdiagonal']:.3e}")
    rule.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

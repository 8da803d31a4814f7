"""The density matrix rho_pq(E) of the tetrahedron method in one eigen-solve (abz_rule_ltm_density_matrix) against the route it
replaces -- ltm_projectors in groups of at most 16 components, ltm_node_weights_dot per group, the matrix composed on the host --
on the same rule and the same resident weights, alternating, in one process.  Profiler off, both routes warmed; wall times are host
clocks around calls that end in a stream synchronisation, the median of `--repeats` repeats of `--calls` calls each; the kernel
times beside them come from the library's own HIP events (ABZ_K_EIG: the eigen-solve kernels of either route; ABZ_K_LTM: the dots
and the final sums) in a separate pass.  Before anything is timed the two routes are compared on the case's own energies.
Cases name:npt with svo or synN (N synthetic bands); the energies are `--nE` values, the first at the Fermi level of one state per
unit cell (svo) or of half filling (synN).
Usage: time_ltm_density_matrix.py [--cases svo:150 svo:48 syn16:24 syn32:16] [--nE 1] [--repeats 5] [--calls 10] [--json FILE]
                                  [--out FILE]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["svo:150", "svo:48", "syn16:24", "syn32:16"])
ap.add_argument("--nE", nargs="+", type=int, default=[1])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--json", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()


def make(name):
    if name == "svo":
        return abz.load_w90_series(os.path.join(ROOT, "tests", "golden", "svo_hr.dat.gz"))
    return abz.synthetic_wannier(int(name[3:]), rmax=2, seed=7)


def groups_of(n):
    """the pairs p <= q (the diagonal first) dealt in order into groups of at most 16 components: DeviceRule.ltm_green_matrix's"""
    todo = [(a, a) for a in range(n)] + [(a, b) for a in range(n) for b in range(a + 1, n)]
    out, ncomp = [[]], 0
    for a, b in todo:
        need = 1 if a == b else 2
        if ncomp + need > L.LTM_MAX_COMP:
            out.append([])
            ncomp = 0
        out[-1].append((a, b))
        ncomp += need
    return out


def group_route(rule, groups):
    n = rule.dev.s.n
    nE = rule.ltm_node_weights_ptr()[2]
    rho = np.zeros((nE, n, n), dtype=np.complex128)
    for group in groups:
        rule.ltm_projectors(group)
        dot = rule.ltm_node_weights_dot()
        c = 0
        for p, q in group:
            if p == q:
                rho[:, p, p] = dot[:, c]
                c += 1
            else:
                rho[:, p, q] = dot[:, c] + 1j * dot[:, c + 1]
                rho[:, q, p] = dot[:, c] - 1j * dot[:, c + 1]
                c += 2
    return rho


def median_ms(fn, ctx, calls):
    """median over the repeats of the mean wall time of a call, ms"""
    fn(); ctx.sync()
    ts = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(calls): fn()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0) / calls)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def kernel_ms(fn, ctx, calls):
    """time of a call's kernels from the library's events, ms: (eigen-solve kernels, dots and final sums)"""
    fn(); ctx.sync()
    ctx.prof_enable(True, kernels=[L.K_EIG, L.K_LTM]); ctx.prof_reset()
    for _ in range(calls): fn()
    ctx.sync()
    eig, _ = ctx.prof_read(L.K_EIG)
    ltm, _ = ctx.prof_read(L.K_LTM)
    ctx.prof_enable(False)
    return eig / calls, ltm / calls


rows, lines = [], []
for case in args.cases:
    name, npt = case.split(":")
    npt = int(npt)
    s = make(name)
    dev = s.device(); ctx = dev.ctx
    n = s.c.shape[-1]
    rule = abz.DeviceRule(dev, npt, None, L.WANT_H | L.WANT_EIG | L.WANT_H_COMPACT)
    groups = groups_of(n)
    E_F, _ = rule.ltm_fermi(1.0 if name == "svo" else 0.5 * n)
    for nE in args.nE:
        Es = E_F + 0.05 * np.arange(nE)
        rule.ltm_node_weights(Es, export=False)
        fused = lambda: rule.ltm_density_matrix()
        route = lambda: group_route(rule, groups)
        a, b = fused(), route()
        dev_ab = float(np.abs(a - b).max())
        calls_r = max(1, args.calls // max(1, len(groups) // 4))
        # the group route right before and right after: the yardstick of this very moment
        r0 = median_ms(route, ctx, calls_r)
        f = median_ms(fused, ctx, args.calls)
        r1 = median_ms(route, ctx, calls_r)
        kf, kr = kernel_ms(fused, ctx, args.calls), kernel_ms(route, ctx, calls_r)
        rmed = 0.5 * (r0[0] + r1[0])
        row = {"series": name, "bands": n, "npt": npt, "nE": nE, "groups": len(groups), "fused_ms": f[0], "fused_min_ms": f[1],
               "fused_max_ms": f[2], "fused_eig_kernel_ms": kf[0], "fused_final_kernel_ms": kf[1], "route_before_ms": r0[0],
               "route_after_ms": r1[0], "route_min_ms": min(r0[1], r1[1]), "route_max_ms": max(r0[2], r1[2]), "route_eig_kernel_ms": kr[0],
               "route_dot_kernel_ms": kr[1], "route_over_fused": rmed / f[0], "max_abs_difference": dev_ab}
        rows.append(row)
        line = (f"DENSMAT {name} n={n} npt={npt} nE={nE}: fused {f[0]:.4f} ms [{f[1]:.4f}, {f[2]:.4f}] (kernels: solve+contract {kf[0]:.4f}, "
                f"final {kf[1]:.4f})  | {len(groups)} group(s) + dot: before {r0[0]:.4f} after {r1[0]:.4f} ms [{row['route_min_ms']:.4f}, "
                f"{row['route_max_ms']:.4f}] (kernels: projectors {kr[0]:.4f}, dots {kr[1]:.4f})  | route / fused = {rmed / f[0]:.2f}, "
                f"max |difference| {dev_ab:.1e}")
        lines.append(line)
        print(line, flush=True)
    rule.close()
if args.json:
    with open(args.json, "w") as fh:
        json.dump(rows, fh, indent=1)
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")

"""The complex integration weights W_b(k; z) of the Green's function (abz_rule_ltm_green_node_weights and its _dot, _fold and
_matrix) against the scans and the projector route they stand beside, on the same rule, alternating, in one process:
  GATHER  the gather per call against the tr G scan (ltm_green) and the one-component weighted scan (ltm_green, elements="energy")
          of the same values of z;
  DOT     the dot of the resident weights against ltm_green(zs, elements="attached") with 4 and 16 attached components;
  FOLD    the fold of an unfolded (cubic) rule;
  MATRIX  G_pq(z) from the resident weights and U(k) (ltm_green_node_weights_matrix, the gathers included) against
          ltm_green_matrix (projector groups + weighted scans).
Profiler off for the wall times: host clocks around calls that end in a stream synchronisation; a window holds as many calls as
fill about `--window` ms (at least one), and the median [min, max] of `--repeats` windows is reported.  The reference route is timed
right before and right after the new one.  Kernel times come from the library's own HIP events (ABZ_K_LTM, ABZ_K_EIG) in a pass of
their own.  Before anything is timed the two routes are compared on the row's own values.
Usage: time_ltm_green_node_weights.py [--gather svo:24 svo:48 svo:150 syn16:24] [--nz 1 8] [--dot svo:48] [--fold svo:48]
                                      [--matrix svo:48 syn16:24 syn32:16] [--mz 1 8 64] [--repeats 5] [--window 100] [--out FILE]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--gather", nargs="*", default=["svo:24", "svo:48", "svo:150", "syn16:24"])
ap.add_argument("--nz", nargs="+", type=int, default=[1, 8])
ap.add_argument("--dot", nargs="*", default=["svo:48"])
ap.add_argument("--fold", nargs="*", default=["svo:48"])
ap.add_argument("--matrix", nargs="*", default=["svo:48", "syn16:24", "syn32:16"])
ap.add_argument("--mz", nargs="+", type=int, default=[1, 8, 64])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window", type=float, default=100.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(line):
    lines.append(line)
    print(line, flush=True)


def make(name):
    if name == "svo":
        return abz.load_w90_series(os.path.join(ROOT, "tests", "golden", "svo_hr.dat.gz"))
    return abz.synthetic_wannier(int(name[3:]), rmax=2, seed=7)


def z_values(rule, nz):
    """nz values across the bands at Im z = 1e-2 (one: the middle of the spectrum)"""
    eig = rule.export(x=False, w=False, eig=True)["eig"]
    lo, hi = float(eig.min()), float(eig.max())
    return (np.array([0.5 * (lo + hi)]) if nz == 1 else np.linspace(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), nz)) + 1e-2j


def timed(fn, ctx):
    """(median, min, max) over the windows of the mean wall time of a call, ms, and the calls per window"""
    fn(); ctx.sync()
    t0 = time.perf_counter(); fn(); ctx.sync()
    calls = int(min(200, max(1, round(args.window / max(1e3 * (time.perf_counter() - t0), 1e-3)))))
    ts = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(calls): fn()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0) / calls)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts)), calls


def kernels(fn, ctx, calls=3):
    """kernel time of a call from the library's events, ms: (ABZ_K_LTM, ABZ_K_EIG)"""
    fn(); ctx.sync()
    ctx.prof_enable(True, kernels=[L.K_EIG, L.K_LTM]); ctx.prof_reset()
    for _ in range(calls): fn()
    ctx.sync()
    ltm, eig = ctx.prof_read(L.K_LTM)[0], ctx.prof_read(L.K_EIG)[0]
    ctx.prof_enable(False)
    return ltm / calls, eig / calls


def fmt(t):
    return f"{t[0]:.4f} ms [{t[1]:.4f}, {t[2]:.4f}] x{t[3]}"


def dev_of(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


for case in args.gather:
    name, npt = case.split(":")
    s = make(name); dev = s.device(); ctx = dev.ctx
    rule = abz.DeviceRule(dev, int(npt), None, L.WANT_EIG)
    eig = rule.export(x=False, w=False, eig=True)["eig"]
    for nz in args.nz:
        zs = z_values(rule, nz)
        gather = lambda: rule.ltm_green_node_weights(zs, export=False)
        trace = lambda: rule.ltm_green(zs)
        energy = lambda: rule.ltm_green(zs, elements="energy")
        if rule.nk * nz <= 48 ** 3 * 8:  # (the export of a larger block is not worth its host memory)
            W = rule.ltm_green_node_weights(zs)
            d0, d1 = dev_of(W.sum(axis=(1, 2)), trace()), dev_of(np.einsum("zkb,kb->z", W, eig), energy()[:, 0])
            del W
        else:
            d0 = d1 = float("nan")
        t0, e0 = timed(trace, ctx), timed(energy, ctx)
        g = timed(gather, ctx)
        t1, e1 = timed(trace, ctx), timed(energy, ctx)
        kg, kt, ke = kernels(gather, ctx)[0], kernels(trace, ctx)[0], kernels(energy, ctx)[0]
        say(f"GATHER {name} n={s.n} npt={npt} nz={nz}: gather {fmt(g)} (kernel {kg:.4f}; per z {g[0] / nz:.4f})  | tr G scan before "
            f"{t0[0]:.4f} after {t1[0]:.4f} ms (kernels {kt:.4f})  | weighted scan, 1 component: before {e0[0]:.4f} after {e1[0]:.4f} ms "
            f"(kernels {ke:.4f})  | gather kernel / weighted scan kernels = {kg / ke:.2f}, / trace kernels = {kg / kt:.2f}; "
            f"|sum W - tr G| {d0:.1e}, |sum e W - G_e| {d1:.1e}")
    rule.close()

for case in args.dot:
    name, npt = case.split(":")
    s = make(name); dev = s.device(); ctx = dev.ctx
    rule = abz.DeviceRule(dev, int(npt), None, L.WANT_EIG)
    zs = z_values(rule, 8)
    rule.ltm_green_node_weights(zs, export=False)
    for ncomp in (4, 16):
        rule.ltm_elements(np.random.default_rng(1).standard_normal((ncomp, rule.nk, s.n)))
        dot = lambda: rule.ltm_green_node_weights_dot()
        scan = lambda: rule.ltm_green(zs, elements="attached")
        d0 = dev_of(dot(), scan())
        s0 = timed(scan, ctx); t = timed(dot, ctx); s1 = timed(scan, ctx)
        say(f"DOT {name} n={s.n} npt={npt} nz=8 ncomp={ncomp}: dot {fmt(t)} (kernels {kernels(dot, ctx)[0]:.4f})  | weighted scan before "
            f"{s0[0]:.4f} after {s1[0]:.4f} ms (kernels {kernels(scan, ctx)[0]:.4f})  | scan / dot = {0.5 * (s0[0] + s1[0]) / t[0]:.1f}, "
            f"max |difference| {d0:.1e}")
    rule.close()

for case in args.fold:
    name, npt = case.split(":")
    s = make(name); dev = s.device(); ctx = dev.ctx
    cub = abz.load_bz(abz.CubicSymIBZ(), np.eye(3))
    src = abz.DeviceRule(dev, int(npt), cub.syms, L.WANT_EIG)
    unf = src.unfold()
    for nz in (1, 8):
        zs = z_values(unf, nz)
        unf.ltm_green_node_weights(zs, export=False)
        fold = lambda: unf.ltm_green_node_weights_fold()
        t = timed(fold, ctx)
        say(f"FOLD {name} n={s.n} npt={npt} cubic ({src.nk} of {unf.nk} nodes) nz={nz}: fold {fmt(t)} (kernel {kernels(fold, ctx)[0]:.4f})")
    unf.close(); src.close()

for case in args.matrix:
    name, npt = case.split(":")
    s = make(name); dev = s.device(); ctx = dev.ctx
    rule = abz.DeviceRule(dev, int(npt), None, L.WANT_H | L.WANT_EIG | L.WANT_H_COMPACT)
    ngroups = 1 if s.n <= 4 else -(-(s.n + s.n * (s.n - 1)) // 16)
    for nz in args.mz:
        zs = z_values(rule, nz)
        fused = lambda: rule.ltm_green_node_weights_matrix(zs)
        route = lambda: rule.ltm_green_matrix(zs)
        d0 = dev_of(fused(), route())
        r0 = timed(route, ctx); f = timed(fused, ctx); r1 = timed(route, ctx)
        kf, kr = kernels(fused, ctx, 1), kernels(route, ctx, 1)
        say(f"MATRIX {name} n={s.n} npt={npt} nz={nz}: from node weights {fmt(f)} (kernels: gather+final {kf[0]:.4f}, solve+contract {kf[1]:.4f})"
            f"  | projector route, ~{ngroups} group(s): before {r0[0]:.4f} after {r1[0]:.4f} ms [{min(r0[1], r1[1]):.4f}, {max(r0[2], r1[2]):.4f}] "
            f"(kernels: scans {kr[0]:.4f}, projectors {kr[1]:.4f})  | route / node weights = {0.5 * (r0[0] + r1[0]) / f[0]:.2f}, "
            f"max |difference| {d0:.1e}")
    rule.ltm_elements(None)
    rule.close()

if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")

"""Pair rules of the tetrahedron method (abz_rule_ltm_pairs): the build of a pair rule without operators (energies only) and with
the 3 velocity operators dH/dkappa_j and the 6 real products a <= b as components, the JDOS scan and the 6-component spectrum scan
over 256 energies on it, abz_rule_ltm_expectation with the same operators and 6 components on the same source rule (the nearest
kernel before pair rules: the same solve, the same loads, no mat-vec and no dots), and the host route (export H and the operator
planes, numpy.linalg.eigh, einsum), in one process.  The source rule holds H and eigenvalues and the operator rules are resident:
neither is part of a device timing (the host route exports them inside its timing: that is its cost).  Wall times are host
clocks around calls that end in a stream synchronisation, after one warm-up call, the median of `--repeats` repeats with the
extremes beside it; the kernel times beside them come from the library's own HIP events (ABZ_K_EIG) in a separate pass.  No
ratio is asserted; the ratio of the two element kernels is printed.
Cases: NAME:NPT:V0,NV,C0,NC with NAME svo (tests/golden/svo_hr.dat.gz) or synN (synthetic_wannier(N, rmax=2, seed=7)).
Usage: time_ltm_pairs.py [--cases svo:48:0,1,1,2 syn16:24:0,8,8,8 syn32:16:8,8,16,8] [--repeats 7] [--host-repeats 1] [--no-host]
       [--out FILE]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["svo:48:0,1,1,2", "syn16:24:0,8,8,8", "syn32:16:8,8,16,8"])
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--host-repeats", type=int, default=1)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def median_ms(fn, ctx, repeats):
    fn(); ctx.sync()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernel_ms(fn, ctx, repeats):
    ctx.prof_enable(True, kernels=[L.K_EIG]); ctx.prof_reset()
    for _ in range(repeats): fn()
    ctx.sync()
    ms = ctx.prof_read(L.K_EIG)[0] / repeats
    ctx.prof_enable(False)
    return ms


PAIRS = [(a, b) for a in range(3) for b in range(a, 3)]


def host_route(rule_h, orules, v0, nv, c0, nc):
    ex = rule_h.export(x=False, w=False, H=True)
    O = [r.export(x=False, w=False, H=True)["H"] for r in orules]
    e, U = np.linalg.eigh(ex["H"])
    Uv, Uc = U[:, :, v0:v0 + nv], U[:, :, c0:c0 + nc]
    M = [np.einsum("kav,kab,kbc->kvc", Uv.conj(), o, Uc) for o in O]
    D = (e[:, None, c0:c0 + nc] - e[:, v0:v0 + nv, None]).reshape(len(e), -1)
    return D, np.stack([(M[a] * M[b].conj()).real.reshape(len(e), -1) for a, b in PAIRS])


say(f"# time_ltm_pairs.py: 3 operators (dH/dkappa_j), 6 components (Re M^a conj(M^b), a <= b), 256 energies; repeats {args.repeats}, "
    f"host repeats {args.host_repeats}")
for case in args.cases:
    name, npt, rng = case.split(":")
    npt = int(npt)
    v0, nv, c0, nc = (int(x) for x in rng.split(","))
    s = abz.load_w90_series(os.path.join(ROOT, "tests", "golden", "svo_hr.dat.gz")) if name == "svo" else abz.synthetic_wannier(int(name[3:]), rmax=2, seed=7)
    n = s.n
    dev = s.device(); ctx = dev.ctx
    ops = abz.velocity_operators(s)
    orules = [o.device(ctx).rule(npt, None, L.WANT_H) for o in ops]
    rule_h = abz.DeviceRule(dev, npt, None, L.WANT_H | L.WANT_EIG)
    comps = [(a, b, "re") for a, b in PAIRS]
    tag = f"PAIRS {name} n={n} npt={npt} ({npt ** 3} nodes) {nv}x{nc} pairs"
    bare = rule_h.ltm_pairs((v0, nv), (c0, nc))
    full = rule_h.ltm_pairs((v0, nv), (c0, nc), orules, comps)
    med, lo, hi = median_ms(bare.refill, ctx, args.repeats)
    say(f"{tag} build, energies only                 : {med:8.3f} ms [{lo:.3f}, {hi:.3f}]")
    med, lo, hi = median_ms(full.refill, ctx, args.repeats)
    kp = kernel_ms(full.refill, ctx, args.repeats)
    say(f"{tag} build, 3 operators / 6 components    : {med:8.3f} ms [{lo:.3f}, {hi:.3f}]  kernel (ABZ_K_EIG events) {kp:.3f} ms")
    fx = lambda: rule_h.ltm_expectation(orules, PAIRS)
    med, lo, hi = median_ms(fx, ctx, args.repeats)
    kx = kernel_ms(fx, ctx, args.repeats)
    say(f"{tag} ltm_expectation 3 ops / 6 components  : {med:8.3f} ms [{lo:.3f}, {hi:.3f}]  kernel (ABZ_K_EIG events) {kx:.3f} ms"
        f"  -> pairs / expectation kernel ratio {kp / kx:.2f}")
    D = full.export(x=False, w=False, eig=True)["eig"]
    ws = np.linspace(D.min(), D.max(), 256)
    med, lo, hi = median_ms(lambda: full.ltm(ws), ctx, args.repeats)
    say(f"{tag} JDOS scan, 256 energies              : {med:8.3f} ms [{lo:.3f}, {hi:.3f}]")
    med, lo, hi = median_ms(lambda: full.ltm(ws, elements="attached"), ctx, args.repeats)
    say(f"{tag} spectrum scan, 6 components x 256    : {med:8.3f} ms [{lo:.3f}, {hi:.3f}]")
    if not args.no_host:
        med, lo, hi = median_ms(lambda: host_route(rule_h, orules, v0, nv, c0, nc), ctx, args.host_repeats)
        say(f"{tag} host (export H and 3 operators + eigh + einsum): {med:8.1f} ms [{lo:.1f}, {hi:.1f}]")
    for r in (bare, full, rule_h):
        r.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

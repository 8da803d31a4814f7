"""Band expectation values as LTM matrix elements: the device route (abz_rule_ltm_expectation, 3 operators -- the derivative
series of H -- and the 6 products a <= b as components) against the host route (export H and the operator planes,
numpy.linalg.eigh, einsum, abz_rule_ltm_elements) and against abz_rule_ltm_orbitals with 6 components on the same rule, in one
process.  The device routes are timed twice: on a rule of eigenvalues only (the call builds a transient H rule) and on a rule
that holds H (the kernel alone).  The operator rules are resident and not part of any timing (the host route exports them
inside its timing: that is its cost).  Wall times are host clocks around calls that end in a stream synchronisation, after
one warm-up call, the median of `--repeats` repeats with the extremes beside it; the kernel time beside them comes from the
library's own HIP events (ABZ_K_EIG) in a separate pass.  The host route runs `--host-repeats` times.  No ratio is asserted.
Usage: time_ltm_expectation.py [--cases syn3:48 syn16:24 syn32:16] [--repeats 7] [--host-repeats 1] [--no-host] [--out FILE]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["syn3:48", "syn16:24", "syn32:16"])
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


def host_route(rule_h, orules):
    H = rule_h.export(x=False, w=False, H=True)["H"]
    O = [r.export(x=False, w=False, H=True)["H"] for r in orules]
    _, U = np.linalg.eigh(H)
    q = [np.einsum("kab,kac,kcb->kb", U.conj(), o, U).real for o in O]
    rule_h.ltm_elements(np.ascontiguousarray(np.stack([q[a] * q[b] for a, b in PAIRS])))


say(f"# time_ltm_expectation.py: 3 operators (dH/dkappa_j), 6 components (products a <= b); repeats {args.repeats}, host repeats {args.host_repeats}")
for case in args.cases:
    name, npt = case.split(":")
    npt, n = int(npt), int(name[3:])
    s = abz.synthetic_wannier(n, rmax=2, seed=7)
    dev = s.device(); ctx = dev.ctx
    ops = abz.velocity_operators(s)
    orules = [o.device(ctx).rule(npt, None, L.WANT_H) for o in ops]
    rule_e = abz.DeviceRule(dev, npt, None, L.WANT_EIG)
    rule_h = abz.DeviceRule(dev, npt, None, L.WANT_H | L.WANT_EIG)
    tag = f"EXPECT n={n} npt={npt} ({npt ** 3} nodes)"
    for key, rule in (("eigenvalue rule (transient H)", rule_e), ("rule with H", rule_h)):
        for what, fn in (("expectation 3 ops / 6 comps", lambda: rule.ltm_expectation(orules, PAIRS)),
                         ("orbitals 6 comps", lambda: rule.ltm_orbitals([0, 1, 2, 0, 1, 2]))):
            med, lo, hi = median_ms(fn, ctx, args.repeats)
            say(f"{tag} {key:30s} {what:28s}: {med:8.3f} ms [{lo:.3f}, {hi:.3f}]  kernel (ABZ_K_EIG events) {kernel_ms(fn, ctx, args.repeats):.3f} ms")
    if not args.no_host:
        med, lo, hi = median_ms(lambda: host_route(rule_h, orules), ctx, args.host_repeats)
        say(f"{tag} host (export H and 3 operators + eigh + einsum + ltm_elements): {med:8.1f} ms [{lo:.1f}, {hi:.1f}]")
    rule_e.close(); rule_h.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

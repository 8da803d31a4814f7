"""The occupied pair scan (abz_rule_ltm_pairs_occupied) against the plain weighted scan (abz_rule_ltm_weighted) of the SAME pair rule,
in one process: 3 velocity operators dH/dkappa_j, the 6 real products a <= b as components, 256 energies, on a grid of `--npt`^3
points of the SrVO3 t2g model (tests/golden/svo_hr.dat.gz).  Two placements of the Fermi level:
  (a) no cell is cut: a synthetic gapped model -- the SVO series with the on-site energy of its third orbital raised by `--shift`, so
      that band 2 is separated from bands 0, 1 -- the pairs (0, 2) x (2, 1), E_F in the gap.  The occupied scan then does the work of
      the plain scan plus its own overhead (two more loads per corner, the classification, two sorts per simplex, no queue);
  (b) the metal: SVO itself at the grid's own Fermi level of `--nstates` states, the pairs (0, 1) x (1, 2).
The JDOS scans (A = 1 against abz_rule_ltm) are timed beside them.  Wall times are host clocks around calls that end in a stream
synchronisation, after one warm-up call, the median of `--repeats` repeats with the extremes beside it; the kernel times come from
the library's own HIP events (ABZ_K_LTM) in a separate pass.  No ratio is asserted; both are printed.
Usage: time_ltm_pairs_occupied.py [--npt 48] [--repeats 7] [--nstates 0.5] [--shift 20] [--out FILE]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--npt", type=int, default=48)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--nstates", type=float, default=0.5)
ap.add_argument("--shift", type=float, default=20.0)
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
    ctx.prof_enable(True, kernels=[L.K_LTM]); ctx.prof_reset()
    for _ in range(repeats): fn()
    ctx.sync()
    ms = ctx.prof_read(L.K_LTM)[0] / repeats
    ctx.prof_enable(False)
    return ms


PAIRS = [(a, b) for a in range(3) for b in range(a, 3)]
svo = abz.load_w90_series(os.path.join(ROOT, "tests", "golden", "svo_hr.dat.gz"))
c = np.array(svo.c)
c[tuple(-f for f in svo.first) + (2, 2)] += args.shift
gapped = abz.FourierSeries(c, period=1.0, first=svo.first, ndim=3)
say(f"# time_ltm_pairs_occupied.py: 3 operators (dH/dkappa_j), 6 components (Re M^a conj(M^b), a <= b), 256 energies, npt = {args.npt}; "
    f"repeats {args.repeats}")
for name, s, lower, upper, nstates in (("(a) gapped, no cell cut", gapped, (0, 2), (2, 1), None), ("(b) SVO metal", svo, (0, 1), (1, 2), args.nstates)):
    dev = s.device(); ctx = dev.ctx
    src = abz.DeviceRule(dev, args.npt, None, L.WANT_EIG)
    pr = src.ltm_pairs(lower, upper, abz.velocity_operators(s), [(a, b, "re") for a, b in PAIRS])
    eig = src.export(x=False, w=False, eig=True)["eig"]
    if nstates is None:
        E_F = 0.5 * (eig[:, lower[0] + lower[1] - 1].max() + eig[:, upper[0]].min())
        assert eig[:, lower[0] + lower[1] - 1].max() < E_F < eig[:, upper[0]].min()
    else:
        E_F = src.ltm_fermi(nstates)[0]
    D = pr.export(x=False, w=False, eig=True)["eig"]
    ws = np.linspace(D.min(), D.max(), 256)
    tag = f"OCC {name} {lower}x{upper} E_F={E_F:.6f}"
    rows = []
    for what, plain, occ in (("spectrum, 6 components", lambda: pr.ltm(ws, elements="attached"), lambda: pr.ltm_occupied(ws, E_F, elements="attached")),
                             ("cumulative, 6 components", lambda: pr.ltm(ws, states=True, elements="attached"),
                              lambda: pr.ltm_occupied(ws, E_F, states=True, elements="attached")),
                             ("JDOS", lambda: pr.ltm(ws), lambda: pr.ltm_occupied(ws, E_F))):
        mp, lp, hp = median_ms(plain, ctx, args.repeats)
        mo, lo, ho = median_ms(occ, ctx, args.repeats)
        kp, ko = kernel_ms(plain, ctx, args.repeats), kernel_ms(occ, ctx, args.repeats)
        say(f"{tag} {what:24s}: plain {mp:7.3f} ms [{lp:.3f}, {hp:.3f}] kernels {kp:.3f} ms | occupied {mo:7.3f} ms [{lo:.3f}, {ho:.3f}] "
            f"kernels {ko:.3f} ms -> ratio {mo / mp:.2f} (kernels {ko / kp:.2f})")
    if nstates is None:  # the two scans agree where no cell is cut
        a, b = pr.ltm(ws, elements="attached"), pr.ltm_occupied(ws, E_F, elements="attached")
        say(f"{tag} max |occupied - plain| = {np.abs(a - b).max():.3e} of {np.abs(a).max():.3e}")
    for r in (pr, src):
        r.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

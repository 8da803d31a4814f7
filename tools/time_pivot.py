"""What ABZ_PIVOT_PARTIAL costs: a dissipative series (both modes are valid on it), 24^3 nodes, 8 swept values; scans of a
cached rule (tr G, G) and the store-free tr G with the mode "none" and "partial" in turn in one process.  Kernel time from
abz_prof_* (the library's own events around its launches), median of REPS runs of each.  Up to 4 bands the scans of a series
that is not Hermitian are the same kernels in both modes."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import autobzcore.jl_amd as abz
from autobzcore.jl_amd import _lib as L

REPS = 5
NPT, ETA, GAMMA = 24, 0.05, 0.1
OMEGAS = np.linspace(-1.0, 1.0, 8)


def dissipative(n, rng):
    """Hermitian hopping on 3^3 coefficients, norm about 1, minus i GAMMA on the diagonal."""
    c = rng.standard_normal((3, 3, 3, n, n)) + 1j * rng.standard_normal((3, 3, 3, n, n))
    c = 0.5 * (c + np.conj(np.swapaxes(c[::-1, ::-1, ::-1], -1, -2))) / np.sqrt(27 * n)
    c[1, 1, 1] += -1j * GAMMA * np.eye(n)
    return abz.FourierSeries(c, period=1.0, first=(-1, -1, -1), ndim=3)


def kernel_ms(ctx, ids, call):
    ctx.prof_reset()
    call()
    ctx.sync()
    return sum(ctx.prof_read(k)[0] for k in ids)


def main():
    rng = np.random.default_rng(11)
    print(f"dissipative series, {NPT}^3 nodes, {len(OMEGAS)} swept values, kernel ms (median of {REPS}): none / partial (ratio)")
    print(f"{'n':>3s}  {'scan tr G':>26s}  {'scan G':>26s}  {'store-free tr G':>26s}")
    for n in (4, 8, 16, 32, 48, 64):
        dev = dissipative(n, rng).device()
        ctx = dev.ctx
        rule = dev.rule(NPT, None, want=L.WANT_H)
        ctx.sync()
        ctx.prof_enable(True)
        jobs = (((L.K_REDUCE,), lambda: rule.reduce(L.F_TRGLOC, [ETA], OMEGAS)),
                ((L.K_REDUCE,), lambda: rule.reduce(L.F_GLOC, [ETA], OMEGAS)),
                ((L.K_CONTRACT, L.K_EVAL), lambda: dev.ptr_sum(NPT, L.F_TRGLOC, [ETA], OMEGAS)))
        ms = {(j, m): [] for j in range(len(jobs)) for m in ("none", "partial")}
        for rep in range(REPS + 1):  # (the first round warms up: code objects, scratch)
            for mode in ("none", "partial"):
                dev.set_pivoting(mode)
                for j, (ids, call) in enumerate(jobs):
                    t = kernel_ms(ctx, ids, call)
                    if rep > 0:
                        ms[(j, mode)].append(t)
        ctx.prof_enable(False)
        cols = []
        for j in range(len(jobs)):
            a, b = np.median(ms[(j, "none")]), np.median(ms[(j, "partial")])
            cols.append(f"{a:8.3f} / {b:8.3f} ({b / a:4.2f})")
        print(f"{n:3d}  " + "  ".join(f"{c:>26s}" for c in cols), flush=True)
        rule.close()
        dev.close()


if __name__ == "__main__":
    main()

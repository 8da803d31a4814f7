"""Rebuild pass of a 3-D SVO rule (H + eigenvalues) with the last contraction inside the grid kernel (the default) and
with level-1 sets in memory (ABZ_EVAL_FUSED=0): wall time per pass over back-to-back rebuilds, arms alternated.

    python3 tools/time_eval_fused.py [--ref-layout] [--pairs | --mirror] [svo | n3gen | n4herm | n4real | n2herm ...] [npt ...]

--pairs: the arms are the two work mappings of the fused grid kernel instead, one grid line per wave (ABZ_EVAL_PAIRS=0)
and one per half-wave wherever the kernel supports it (ABZ_EVAL_PAIRS=2).
--mirror: the arms are every plane evaluated (ABZ_EVAL_MIRROR=0) and, for real Hermitian series (svo, n4real), the planes
k3 <= npt/2 evaluated and stored a second time as H(-k) = conj H(k), also where the size rule would not (ABZ_EVAL_MIRROR=2).
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import autobzcore.jl_amd as abz
L = abz._lib


def synthetic(dims, n, hermitian, real=False):
    rng = np.random.default_rng(7)
    c = rng.standard_normal(dims + (n, n)) + (0 if real else 1j) * rng.standard_normal(dims + (n, n))
    if hermitian:
        c = 0.5 * (c + np.conj(np.swapaxes(c[::-1, ::-1, ::-1], -1, -2)))
    return abz.FourierSeries(c, period=1.0, first=tuple(-(m // 2) for m in dims), ndim=3)


SERIES = {
    "svo": lambda: abz.load_w90_series(os.path.join(ROOT, "tests", "golden", "svo_hr.dat.gz")),  # 3 bands, Hermitian, 11^3
    "n3gen": lambda: synthetic((6, 6, 6), 3, False),  # unpacked rows, two waves per SIMD
    "n4herm": lambda: synthetic((7, 7, 7), 4, True),
    "n4real": lambda: synthetic((7, 7, 7), 4, True, real=True),  # c(-R) = c(R)^T, real: H(-k) = conj H(k)
    "n2herm": lambda: synthetic((9, 9, 9), 2, True),
}


def per_pass(ctx, rule, n):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        rule.rebuild()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / n


args = sys.argv[1:]
ref_layout = "--ref-layout" in args  # full matrices (168 B per k-point at 3 bands) instead of the upper triangle of Hermitian rules
pairs = "--pairs" in args
mirror = "--mirror" in args
args = [a for a in args if a not in ("--ref-layout", "--pairs", "--mirror")]
names = [a for a in args if a in SERIES] or ["svo"]
npts = [int(a) for a in args if a not in SERIES] or [64, 100, 128, 150, 200, 250, 400]
# (switch, value of the base arm, value of the new arm, their names)
switch, base, new, base_name, new_name = (("ABZ_EVAL_PAIRS", "0", "2", "line per wave", "line per half-wave") if pairs else
                                          ("ABZ_EVAL_MIRROR", "0", "2", "every plane", "mirrored") if mirror else
                                          ("ABZ_EVAL_FUSED", "0", "1", "level-1 sets in memory", "fused"))
for name in names:
    dev = SERIES[name]().device()
    herm = name != "n3gen"
    for npt in npts:
        want = L.WANT_H | (L.WANT_EIG if herm else 0)
        rule = abz.DeviceRule(dev, npt, None, want if ref_layout else dev._layout_want(want))
        n = max(8, min(256, int(2e9 / npt**3)))
        res = {new: [], base: []}
        for rep in range(4):  # the first round warms up
            for arm in (base, new):
                os.environ[switch] = arm
                t = per_pass(dev.ctx, rule, n)
                if rep:
                    res[arm].append(t)
        del os.environ[switch]
        off, on = sorted(res[base]), sorted(res[new])
        print(f"{name}{' ref-layout' if ref_layout else ''} npt {npt}: {base_name} {off[0]:.4f} {off[1]:.4f} {off[2]:.4f} ms, {new_name} {on[0]:.4f} {on[1]:.4f} {on[2]:.4f} ms "
              f"per pass ({n} passes per sample); medians {off[1]:.4f} -> {on[1]:.4f} ({100 * (on[1] / off[1] - 1):+.1f} %)", flush=True)
        rule.close()
    dev.drop_rules()

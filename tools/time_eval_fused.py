"""Rebuild pass of a 3-D SVO rule (H + eigenvalues) with the last contraction inside the grid kernel (the default) and
with level-1 sets in memory (ABZ_EVAL_FUSED=0): wall time per pass over back-to-back rebuilds, arms alternated.

    python3 tools/time_eval_fused.py [--ref-layout] [--pairs | --mirror | --passwave] [svo | n3gen | n3herm | n4herm | n4real | n2herm ...] [npt ...]

--pairs: the arms are the two work mappings of the fused grid kernel instead, one grid line per wave (ABZ_EVAL_PAIRS=0)
and one per half-wave wherever the kernel supports it (ABZ_EVAL_PAIRS=2).
--mirror: the arms are every plane evaluated (ABZ_EVAL_MIRROR=0) and, for real Hermitian series (svo, n4real), the planes
k3 <= npt/2 evaluated and stored a second time as H(-k) = conj H(k), also where the size rule would not (ABZ_EVAL_MIRROR=2).
--passwave: three arms, all of the fused kernel: the launcher's choice of mapping with a pair of lines per wave where it takes
pairs (ABZ_EVAL_PASSWAVE=0), one pass of a pair per wave wherever the kernel supports it (ABZ_EVAL_PAIRS=2 and
ABZ_EVAL_PASSWAVE=2; elsewhere the pair mapping as it is) and one grid line per wave (ABZ_EVAL_PAIRS=0).
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
    "n3herm": lambda: synthetic((7, 7, 7), 3, True),  # complex Hermitian: never mirrored
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
passwave = "--passwave" in args
args = [a for a in args if a not in ("--ref-layout", "--pairs", "--mirror", "--passwave")]
names = [a for a in args if a in SERIES] or ["svo"]
npts = [int(a) for a in args if a not in SERIES] or [64, 100, 128, 150, 200, 250, 400]
# the arms, the base arm first: (environment, name)
ARMS = ([({"ABZ_EVAL_PASSWAVE": "0"}, "pair per wave"), ({"ABZ_EVAL_PAIRS": "2", "ABZ_EVAL_PASSWAVE": "2"}, "pass per wave"), ({"ABZ_EVAL_PAIRS": "0"}, "line per wave")] if passwave else
        [({"ABZ_EVAL_PAIRS": "0"}, "line per wave"), ({"ABZ_EVAL_PAIRS": "2"}, "line per half-wave")] if pairs else
        [({"ABZ_EVAL_MIRROR": "0"}, "every plane"), ({"ABZ_EVAL_MIRROR": "2"}, "mirrored")] if mirror else
        [({"ABZ_EVAL_FUSED": "0"}, "level-1 sets in memory"), ({"ABZ_EVAL_FUSED": "1"}, "fused")])
for name in names:
    dev = SERIES[name]().device()
    herm = name != "n3gen"
    for npt in npts:
        want = L.WANT_H | (L.WANT_EIG if herm else 0)
        rule = abz.DeviceRule(dev, npt, None, want if ref_layout else dev._layout_want(want))
        n = max(8, min(256, int(2e9 / npt**3)))
        res = [[] for _ in ARMS]
        for rep in range(4):  # the first round warms up
            for i, (env, _) in enumerate(ARMS):
                os.environ.update(env)
                t = per_pass(dev.ctx, rule, n)
                for k in env:
                    del os.environ[k]
                if rep:
                    res[i].append(t)
        res = [sorted(r) for r in res]
        off = res[0]
        line = f"{name}{' ref-layout' if ref_layout else ''} npt {npt}: " + ", ".join(
            f"{arm_name} {r[0]:.4f} {r[1]:.4f} {r[2]:.4f} ms" for (_, arm_name), r in zip(ARMS, res))
        print(line + f" per pass ({n} passes per sample); medians {off[1]:.4f}" +
              "".join(f" -> {r[1]:.4f} ({100 * (r[1] / off[1] - 1):+.1f} %)" for r in res[1:]), flush=True)
        rule.close()
    dev.drop_rules()

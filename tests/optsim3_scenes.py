"""Seeded OptimizeSim3 problems on top of sim3_scenes.make_problem, and the case table shared by
tests/test_optsim3.py and tests/test_optsim3_shim.py, with the literal's runs computed once per
process."""
import functools

import numpy as np

import optsim3_literal as lit
import sim3_scenes

F32 = np.float32
INV_LEVEL_SIGMA2 = [F32(1) / s for s in sim3_scenes.LEVEL_SIGMA2]  # mvInvLevelSigma2 (float division)
TH2 = 10.0  # LoopClosing::ComputeSim3 passes th2 = 10 (src/LoopClosing.cc:427)


def _pinhole(X, K):
    X = np.asarray(X, np.float64)
    return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], axis=1)


def make_problem(N, outliers, fix_scale, seed, pixel_noise=0.5, rot=0.01, trans=0.02, dscale=0.02, noise3d=0.0,
                 same_K=False):
    """N correspondences of sim3_scenes.make_problem (X1 = s R X2 + t; the share `outliers` of set 2
    unrelated = gross outliers) with their projections + pixel noise scaled by the octave's sigma,
    mixed octaves, and a start S12 perturbed from the truth by a rotation of `rot` rad, `trans` in
    translation and a relative `dscale` in scale (none with fix_scale)."""
    P = sim3_scenes.make_problem(N, outliers, fix_scale, seed, noise=noise3d)
    g = np.random.RandomState(seed + 77777)
    s, R, t = P["truth"]
    K1 = sim3_scenes.K1
    K2 = K1 if same_K else sim3_scenes.K2
    o1, o2 = g.randint(0, 8, N), g.randint(0, 8, N)
    sig1 = np.array([np.sqrt(float(sim3_scenes.LEVEL_SIGMA2[o])) for o in o1]).reshape(-1, 1)
    sig2 = np.array([np.sqrt(float(sim3_scenes.LEVEL_SIGMA2[o])) for o in o2]).reshape(-1, 1)
    obs1 = _pinhole(P["x3dc1"], K1) + g.normal(size=(N, 2)) * pixel_noise * sig1
    obs2 = _pinhole(P["x3dc2"], K2) + g.normal(size=(N, 2)) * pixel_noise * sig2
    Rp = sim3_scenes.rotation(g.normal(size=3), rot) @ R
    tp = t + g.normal(size=3) * trans
    sp = s if fix_scale else s * (1.0 + dscale * g.normal())
    S12 = lit.sim3_from_rts(Rp, tp, sp)
    n_out = int(round(outliers * N))
    return {"x3dc1": P["x3dc1"], "x3dc2": P["x3dc2"], "obs1": obs1.astype(F32), "obs2": obs2.astype(F32),
            "inv_sigma2_1": np.array([INV_LEVEL_SIGMA2[o] for o in o1], F32),
            "inv_sigma2_2": np.array([INV_LEVEL_SIGMA2[o] for o in o2], F32),
            "K1": K1, "K2": K2, "S12": S12, "th2": TH2, "bFixScale": bool(fix_scale), "truth": (s, R, t),
            "n_outliers": n_out, "octave1": o1, "octave2": o2}


def gross(P):
    """The correspondences whose set-2 point is unrelated to its set-1 point (3-D residual under the truth)."""
    s, R, t = P["truth"]
    X1 = P["x3dc1"].astype(np.float64)
    X2 = P["x3dc2"].astype(np.float64)
    return np.linalg.norm(X1 - (s * X2 @ R.T + t), axis=1) > 0.2


# ------------------------------------------------------------------ the GPU case table
# name -> make_problem arguments.  Shapes: the smallest at which the kernel takes another path (0; 9 and
# 10 around the early return; 32 pairs = 64 edges = one wave and 33; 64 and 65; 128 pairs = 256 edges =
# one staging chunk and 129 = two; 300 pairs = three staging chunks and two passes of the 256-pair
# outlier scan), fix_scale 0/1, K1 != K2 everywhere except one same-K case, no outliers (nMore = 5),
# 30 % (nMore = 10), too many (< 10 survivors), far starts (rejected trials).  Seeds: 3000 + N, except
# the far, stale and partial-nulling cases, whose seeds were searched on the CPU with the literal alone
# (the first of a range with the wanted counters; test_optsim3.py asserts them).
CASES = {
    "n0": dict(N=0, outliers=0.0, fix_scale=0, seed=3000),
    "n9_early": dict(N=9, outliers=0.0, fix_scale=0, seed=3009),
    "n10": dict(N=10, outliers=0.0, fix_scale=0, seed=3010),
    "n11_fix": dict(N=11, outliers=0.0, fix_scale=1, seed=3011),
    "n32": dict(N=32, outliers=0.0, fix_scale=0, seed=3032),
    "n33_out30_fix": dict(N=33, outliers=0.3, fix_scale=1, seed=3033),
    "n64_out30": dict(N=64, outliers=0.3, fix_scale=0, seed=3064),
    "n65": dict(N=65, outliers=0.0, fix_scale=1, seed=3065),
    "n128_out30": dict(N=128, outliers=0.3, fix_scale=0, seed=3128),
    "n129_out30_fix": dict(N=129, outliers=0.3, fix_scale=1, seed=3129),
    "n300_out30": dict(N=300, outliers=0.3, fix_scale=0, seed=3300),
    "n300_sameK_fix": dict(N=300, outliers=0.0, fix_scale=1, seed=3301, same_K=True),
    "n40_out80_early": dict(N=40, outliers=0.8, fix_scale=0, seed=3040),  # every pair nulled
    "n14_early_partial": dict(N=14, outliers=0.36, fix_scale=0, seed=3015),  # 5 nulled, 9 survive: return 0
    "n65_far": dict(N=65, outliers=0.3, fix_scale=0, seed=3072, rot=0.2, trans=0.3, dscale=0.2),
    "n129_far_fix": dict(N=129, outliers=0.3, fix_scale=1, seed=3130, rot=0.3, trans=0.5),
    "n33_stale_fix": dict(N=33, outliers=0.1, fix_scale=1, seed=5008, pixel_noise=0.1),
}
# what the literal must report for the named cases (asserted on the CPU in test_optsim3.py)
FAR = ("n65_far", "n129_far_fix")            # rejected trials
STALE = ("n33_stale_fix", "n300_sameK_fix")  # the last trial of optimize(5) rejected
EARLY = ("n0", "n9_early", "n40_out80_early", "n14_early_partial")


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, the literal's result) of one table case; computed once, never modified."""
    P = make_problem(**CASES[name])
    return P, lit.optimize_sim3(P)


def batch_problems():
    """24 mixed problems for the device batch."""
    out = []
    for b in range(24):
        N = (0, 9, 12, 31, 64, 65, 97, 130)[b % 8] + (b // 8)
        out.append(make_problem(N, (0.0, 0.3, 0.8)[b % 3], b % 2, 4000 + b,
                                **(dict(rot=0.3, trans=0.5) if b % 5 == 4 else {})))
    return out

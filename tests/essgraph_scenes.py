"""Scenes for tests/test_essgraph.py: a ring of keyframes whose odometry drifted, closed by a loop correction,
as the map description Optimizer.OptimizeEssentialGraph takes.

The camera drives once round a circle; the estimated trajectory composes the true relative motions with a
per-step noise and a deliberate bias (yaw, and scale unless bFixScale), so the last keyframe (pCurKF) misses
the first ones by far more than the noise.  The loop correction gives pCurKF and its two predecessors their
true poses as Sim3 (CorrectedSim3; NonCorrectedSim3 holds their drifted ones), as LoopClosing::CorrectLoop
does before it calls the optimiser.  Around that, everything the edge selection branches on:

* a spanning tree to the previous keyframe; covisibility weights 300 / 150 (kept) and 80 (below minFeat);
* an old loop edge between two far keyframes (a long envelope row);
* LoopConnections holding (pCurKF, pLoopKF) with weight 60 (the minFeat exception), a pair with weight 50
  (dropped), a pair that is also covisible (the sInsertedEdges skip) and the pair (pCurKF's parent, pCurKF),
  whose block the spanning-tree edge also writes, transposed;
* one bad keyframe that its neighbours still list as a covisible, one bad point, points corrected by pCurKF
  and points that are not.

Sizes: n = 2 (one edge, 7 unknowns), n = 3 (the duplicate, transposed pair), n = 12, n = 40 (273 unknowns).
"""
import functools

import numpy as np

import essgraph_literal as lit

F32 = np.float32
STEP_ROT = 2e-4     # per-step odometry noise: rotation vector sigma (rad)
STEP_TRANS = 2e-3   # ... translation sigma (m)
RADIUS = 5.0


def rot(v):
    v = np.asarray(v, float)
    th = np.linalg.norm(v)
    if th < 1e-12:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _se3(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def true_poses(n):
    """Tcw of n cameras round a circle (the last one a step short of the first)."""
    out = []
    for i in range(n):
        a = 2 * np.pi * i / n
        Rwc = rot([0, 0, a]) @ rot([0.1 * np.sin(3 * a), 0, 0])
        twc = np.array([RADIUS * np.cos(a), RADIUS * np.sin(a), 0.2 * np.sin(2 * a)])
        out.append(np.linalg.inv(_se3(Rwc, twc)))
    return out


def make_scene(n, fix_scale, seed, n_points=240):
    """n good keyframes (n >= 2).  Returns the map description M with M["truth"] = {id: Tcw 4x4}."""
    rng = np.random.RandomState(seed)
    with_bad = n >= 12
    total = n + (1 if with_bad else 0)
    bad_at = total // 2 if with_bad else -1
    ids = list(range(total))
    good = [i for i in ids if i != bad_at]
    T_true = true_poses(total)
    yaw_bias = 0.0 if n < 4 else 0.08 / total
    scale_bias = 0.0 if fix_scale else 0.15 / total
    T_est = [T_true[0].copy()]
    for i in range(1, total):
        rel = T_true[i] @ np.linalg.inv(T_true[i - 1])
        noise = _se3(rot(rng.normal(0, STEP_ROT, 3) + [0, 0, yaw_bias]), rng.normal(0, STEP_TRANS, 3))
        rel = noise @ rel
        rel[:3, 3] *= 1 + scale_bias * i
        T_est.append(rel @ T_est[i - 1])
    T_est = [T.astype(F32) for T in T_est]
    cur = good[-1]
    loop = good[0] if n < 4 else good[1]
    prev_good = {g: (good[k - 1] if k > 0 else None) for k, g in enumerate(good)}
    next_good = {g: (good[k + 1] if k + 1 < len(good) else None) for k, g in enumerate(good)}

    def weight(i, j):
        d = abs(i - j)
        return {1: 300, 2: 150, 3: 80}.get(d, 0)
    extra = {}  # symmetric extra covisibilities the loop fusion created
    if n >= 4:
        extra[(cur, loop)] = 60
        extra[(cur, loop + 1)] = 120
        extra[(good[-2], loop)] = 50
    elif n == 3:
        extra[(cur, loop)] = 60
    old_loop = (good[-3], good[2]) if n >= 12 else None
    kfs = []
    for i in ids:
        cov = {}
        for j in ids:
            if j != i and weight(i, j):
                cov[j] = weight(i, j)
        for (a, b), w in extra.items():
            if i == a:
                cov[b] = w
            if i == b:
                cov[a] = w
        order = sorted(cov.items(), key=lambda kv: (-kv[1], kv[0]))
        parent = prev_good.get(i) if i != bad_at else i - 1
        children = {next_good[i]} if i in next_good and next_good[i] is not None else set()
        loops = set()
        if old_loop and i in old_loop:
            loops = {old_loop[0] if i == old_loop[1] else old_loop[1]}
        kfs.append({"id": i, "Tcw": T_est[i][:3, :4].copy(), "parent": parent, "children": children,
                    "loop_edges": loops, "covisibles": order, "bad": i == bad_at})
    # the loop correction: pCurKF and its predecessors get their true poses, at the drifted map's scale
    k = 1.0 if fix_scale else float(np.linalg.norm(np.linalg.inv(T_est[cur])[:3, 3] - np.linalg.inv(T_est[good[-2]])[:3, 3])
                                    / np.linalg.norm(np.linalg.inv(T_true[cur])[:3, 3]
                                                     - np.linalg.inv(T_true[good[-2]])[:3, 3]))
    corrected, noncorrected = {}, {}
    if n >= 3:
        for i in good[-3:] if n >= 4 else [cur]:
            q = lit.sim3_from_tcw(T_true[i].astype(F32)[:3, :4])
            q[4:7] *= k
            q[7] = k
            corrected[i] = q
            noncorrected[i] = lit.sim3_from_tcw(T_est[i][:3, :4])
    else:  # n == 2: the current keyframe alone, no LoopConnections: the one spanning-tree edge pulls it back
        q = lit.sim3_from_tcw(T_true[cur].astype(F32)[:3, :4])
        q[4:7] += [0.02, -0.01, 0.015]
        corrected[cur] = q
        noncorrected[cur] = lit.sim3_from_tcw(T_est[cur][:3, :4])
    conn = {}
    if n >= 4:
        conn = {cur: {loop, loop + 1}, good[-2]: {loop, cur}}
    elif n == 3:
        conn = {cur: {loop}, good[1]: {cur}}
    points = []
    for p in range(n_points):
        ref = good[rng.randint(len(good))]
        Xc = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 6)])
        Twc = np.linalg.inv(T_est[ref].astype(float))
        pos = (Twc[:3, :3] @ Xc + Twc[:3, 3]).astype(F32)
        by_cur = p % 5 == 0 and bool(corrected)
        points.append({"pos": pos, "ref": ref, "mnCorrectedByKF": cur if by_cur else 0,
                       "mnCorrectedReference": list(corrected)[p % len(corrected)] if by_cur else 0,
                       "bad": p == 7})
    return {"keyframes": kfs, "pLoopKF": loop, "pCurKF": cur, "NonCorrectedSim3": noncorrected,
            "CorrectedSim3": corrected, "LoopConnections": conn, "bFixScale": bool(fix_scale), "points": points,
            "truth": {i: T_true[i] for i in ids}, "map_scale": k}


SIZES = (2, 3, 12, 40)
CASES = {"n%d_%s" % (n, "fix" if f else "free"): (n, f, 100 + 7 * n + f) for n in SIZES for f in (1, 0)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(map description, the literal's result), computed once and shared; treat both as read-only."""
    n, f, seed = CASES[name]
    M = make_scene(n, f, seed)
    return M, lit.optimize_essential_graph(M)


# the n = 12 scene's edges, listed by hand from make_scene's rules (ids 0..12, 6 bad, pLoopKF 1, pCurKF 12):
EXPECTED_N12 = (
    # LoopConnections in ascending id: 11 -> {1 (weight 50: dropped), 12}; 12 -> {1 (the exception), 2}
    [(11, 12, 0), (12, 1, 0), (12, 2, 0)]
    # per keyframe in ascending id: parent, old loop edges to smaller ids, covisibles >= 100 by weight then id
    + [(1, 0, 1)]
    + [(2, 1, 1), (2, 0, 1)]
    + [(3, 2, 1), (3, 1, 1)]
    + [(4, 3, 1), (4, 2, 1)]
    + [(5, 4, 1), (5, 3, 1)]
    # 6 is bad; 7's parent is 5 (so the weight-150 covisible 5 is its parent), its covisible 6 is bad
    + [(7, 5, 1)]
    + [(8, 7, 1)]            # 8's weight-150 covisible 6 is bad
    + [(9, 8, 1), (9, 7, 1)]
    + [(10, 9, 1), (10, 2, 1), (10, 8, 1)]   # the old loop edge (10, 2) between parent and covisibles
    + [(11, 10, 1), (11, 9, 1)]
    + [(12, 11, 1), (12, 10, 1)]             # 12's covisible 2 (weight 120) is in sInsertedEdges: skipped
)

"""Candidate sets for k_octree's count-pyramid path, built with tests/octree_scenes.py's helpers.  A scene
carries `condition`, which asserts on the model (tests/octree_pyramid_model.py), the literal's trace and
the plan items that it takes the path it is named for; no condition reads the kernel.

The plan's depth D comes from ORBX_LP_OCT_PYRAMID (one row per ORBX_LP_OCTREE row).  A scene that depends
on D is built for the D of the launch group it is to run under in a batch of three; the one-launch row of
smaller batches has D = 0 (the generic path alone), so a batch of one image takes path 2 on every level
that holds a candidate.

A note on reaching depth D: two candidates one pixel apart in an otherwise empty root do NOT get there.
Their root splits into one child that holds both, the list does not grow, and DistributeOctTree stops on
`size == prevSize` after the first round (the scene `pair-stuck` of octree_scenes).  The list has to grow
in every round on the way down, so the cap scenes put one more candidate into a sibling box at every depth
(a ladder) and the tight pair at the bottom."""
import functools

import numpy as np

import octree_literal as lit
import octree_pyramid_model as model
import octree_scenes as sc
from orb_slam2_commit_amd import _lib
from orb_slam2_commit_amd.orb import debug_launch_plan

LP_OCT_PYRAMID = 13


@functools.lru_cache(maxsize=None)
def pyramid_rows(g):
    return debug_launch_plan(_lib.ExtractorParams(*g.params), g.w, g.h, LP_OCT_PYRAMID).reshape(-1, 8)


def plan_depth(g, l, n_img):
    """D of the launch row level l runs under in a batch of n_img images."""
    rows = pyramid_rows(g)
    one = g.groups[-1]
    if n_img <= one[7]:
        return int(rows[-1][0])
    return int(next(r for r, q in zip(rows[:-1], g.groups[:-1]) if q[0] <= l < q[1])[0])


def model_level(g, l, pts, D):
    minBX, minBY, maxBX, maxBY, N, _ = g.box(l)
    return model.run(pts[:, 0] - minBX, pts[:, 1] - minBY, pts[:, 2], minBX, maxBX, minBY, maxBY, N, D)


@functools.lru_cache(maxsize=None)
def expected_paths(s, n_img, depth_cap=-1):
    """The model's path per level for scene s in a batch of n_img images."""
    out = []
    for l in range(s.g.nlevels):
        D = plan_depth(s.g, l, n_img)
        if depth_cap >= 0:
            D = min(D, depth_cap)
        out.append(model_level(s.g, l, s.ordered[l], D)[1])
    return np.array(out, np.int32)


# ------------------------------------------------------------------------------------------- scenes
def _ladder(g, l, depth, tight):
    """A ladder down to a box of depth `depth` - 1 on level l: one candidate in a sibling box at every depth
    1..depth-1 and two in the box at the bottom -- in two of its children (tight False: the box of depth
    `depth` - 1 is the deepest node split), or in ONE child, a box of depth `depth` (tight True: that child
    is selected for splitting too).  Relative (x, y)."""
    mask = sc.allowed_mask(g, l)
    H, W = mask.shape
    box = lit.leaves(W, H, 0)[len(lit.leaves(W, H, 0)) // 2]
    xy = []
    for d in range(1, depth):
        kids = lit.child_boxes(*box)
        kids.sort(key=lambda c: -int(mask[c[1]:c[3], c[0]:c[2]].sum()))
        xy.append(sc.in_leaf(mask, kids[1], 1)[0])  # the rung
        box = kids[0]
    kids = lit.child_boxes(*box)
    kids.sort(key=lambda c: -int(mask[c[1]:c[3], c[0]:c[2]].sum()))
    if tight:
        xy += list(sc.in_leaf(mask, kids[0], 2))
    else:
        xy += [sc.in_leaf(mask, kids[0], 1)[0], sc.in_leaf(mask, kids[1], 1)[0]]
    return np.array(xy)


def scene_cap(w, h, nfeat, n_img, tight, params=sc.P1):
    g = sc.geom(w, h, (nfeat,) + params)
    D = plan_depth(g, 0, n_img)
    xy = _ladder(g, 0, D, False) if not tight else _ladder(g, 0, D + 1, False)
    # cap_exact: the pair separates at depth D (its box of depth D - 1 splits); cap_plus_one: one level
    # tighter, the pair shares a box of depth D and separates below it
    pts = {0: sc.pts3(g, 0, xy, 10 + 7 * np.arange(len(xy)))}
    name = "%s-%dx%d-n%d" % ("cap_plus_one" if tight else "cap_exact", w, h, n_img)

    def condition(s):
        r = s.literal[0]
        assert set(r["final_sizes"]) == {1} and all(e["phase"] == 1 for e in r["trace"]), r["trace"]
        idx, path, deepest = model_level(g, 0, s.ordered[0], D)
        assert np.array_equal(idx, r["index"])
        assert (path, deepest) == ((2, D) if tight else (1, D - 1)), (path, deepest, D)
        if tight and D < model.MAX_DEPTH:
            assert model_level(g, 0, s.ordered[0], D + 1)[1:] == (1, D)
    return sc.Scene(name, g, pts, condition)


def scene_mixed():
    """In one image: a cap_plus_one level, ordinary levels and an empty level."""
    g = sc.geom(320, 240, (500,) + sc.P8)
    rng = np.random.default_rng(21)
    D0 = plan_depth(g, 0, 3)
    xy = _ladder(g, 0, D0 + 1, False)
    pts = {0: sc.pts3(g, 0, xy, 10 + 7 * np.arange(len(xy)))}
    for l in (1, 3, 4, 5, 6, 7):
        pts[l] = sc.random_points(g, l, min(len(g.region(l)[0]) // 12, 400), rng)

    def condition(s):
        p = expected_paths(s, 3)
        assert p[0] == 2 and p[2] == 0 and set(p[[1, 3, 4, 5, 6, 7]]) == {1}, p
        p = expected_paths(s, 1)  # the one-launch row runs the generic path alone
        assert p[2] == 0 and set(np.delete(p, 2)) == {2}, p
    return sc.Scene("mixed", g, pts, condition)


def scene_boundaries(w, h, n_img):
    """Around the split point of boxes of every depth 0..D-1, odd-sized ones first: the four pixels
    (x0 + hx - 1 | x0 + hx) x (y0 + hy - 1 | y0 + hy), one per child, two on each boundary."""
    g = sc.geom(w, h, (1500,) + sc.P1)
    D = plan_depth(g, 0, n_img)
    mask = sc.allowed_mask(g, 0)
    H, W = mask.shape
    xy, odd_by_depth, taken = [], {}, set()
    minBX, minBY, maxBX, maxBY = g.box(0)[:4]

    def boxes_of(quad):  # the quad's boxes of depth D
        d = model.Descent([q[0] for q in quad], [q[1] for q in quad], minBX, maxBX, minBY, maxBY)
        gx, gy = d.depth(D)
        return {(int(a), int(b)) for a, b in zip(gx, gy)}

    for depth in range(D):
        boxes = lit.leaves(W, H, depth)
        boxes.sort(key=lambda b: -(((b[2] - b[0]) % 2) + ((b[3] - b[1]) % 2)))
        n = 0
        for b in boxes:
            x0, y0, x1, y1 = b
            (_, _, bx, by) = lit.child_boxes(*b)[0]
            quad = [[bx - 1, by - 1], [bx, by - 1], [bx - 1, by], [bx, by]]
            if not all(x0 <= x < x1 and y0 <= y < y1 and mask[y, x] for x, y in quad):
                continue
            keys = boxes_of(quad)
            if len(keys) < 4 or keys & taken:  # one candidate per box of depth D: nothing splits below D - 1
                continue
            taken |= keys
            xy += quad
            odd_by_depth[depth] = odd_by_depth.get(depth, 0) + ((x1 - x0) % 2) + ((y1 - y0) % 2)
            n += 1
            if n == 3:
                break
    xy = np.unique(np.array(xy), axis=0)
    pts = {0: sc.pts3(g, 0, xy, 1 + (np.arange(len(xy)) * 37) % 250)}

    def condition(s):
        # a split on every depth; odd-sized boxes where the geometry has them (320 x 240: a 288 x 208 border
        # box, odd from depth 4 on)
        assert sorted(odd_by_depth) == list(range(D)) and sum(odd_by_depth.values()) >= 3, odd_by_depth
        r = s.literal[0]
        idx, path, deepest = model_level(g, 0, s.ordered[0], D)
        assert np.array_equal(idx, r["index"]) and path == 1 and deepest == D - 1, (path, deepest, D)
        assert set(r["final_sizes"]) == {1}
    return sc.Scene("boundaries-%dx%d-n%d" % (w, h, n_img), g, pts, condition)


def scene_root_edges(w, h, n_ini):
    """Candidates on both sides of every root edge (int)(hX * i), where the root a candidate is filed
    under, (int)(x / hX), and the root box that contains it can differ; and in the last column."""
    g = sc.geom(w, h, (1500,) + sc.P1)
    mask = sc.allowed_mask(g, 0)
    H, W = mask.shape
    _, n, hX = lit.root_count(0, W, 0, H)
    xs = sorted({int(hX * np.float32(i)) + d for i in range(1, n) for d in (-2, -1, 0, 1, 2)} | {int(np.flatnonzero(mask.any(0)).max())})
    xy = []
    for x in xs:
        ys = np.flatnonzero(mask[:, x])
        xy += [[x, int(ys[len(ys) // 5])], [x, int(ys[len(ys) // 2])], [x, int(ys[4 * len(ys) // 5])]]
    xy = np.array(xy)
    pts = {0: sc.pts3(g, 0, xy, 1 + (np.arange(len(xy)) * 53) % 250)}

    def condition(s):
        r = s.literal[0]
        assert r["nIni"] == n_ini == n == g.box(0)[5]
        x = s.ordered[0][:, 0] - g.box(0)[0]
        filed = (x.astype(np.float32) / hX).astype(np.int64)
        edges = np.array([int(hX * np.float32(i)) for i in range(n + 1)])
        inside = np.searchsorted(edges, x, side="right") - 1
        assert filed.max() == n - 1 and len(set(filed)) == n
        assert (filed == inside).any() and ((x[:, None] == edges[None, 1:-1]).any(1)).sum() >= 3 * (n - 1)
        for D in range(1, model.MAX_DEPTH + 1):
            assert np.array_equal(model_level(g, 0, s.ordered[0], D)[0], r["index"]), D
    return sc.Scene("root_edges-%d" % n_ini, g, pts, condition)


def scene_kitti():
    """1241 x 376 (nIni = 4), ordinary candidates on every level but the fourth, and on level 3 a ladder whose
    pair shares a box of the depth D of level 3's launch group: in a batch of three that block leaves the
    pyramid path."""
    g = sc.geom(1241, 376, (2000,) + sc.P8)
    tight_depth = plan_depth(g, 3, 3)
    rng = np.random.default_rng(22)
    pts = {}
    for l in range(g.nlevels):
        pts[l] = sc.random_points(g, l, min(len(g.region(l)[0]) // 60, 2500), rng)
    xy = _ladder(g, 3, tight_depth + 1, False)
    lad = sc.pts3(g, 3, xy, 10 + 7 * np.arange(len(xy)))
    pts[3] = lad  # alone on its level: among ordinary candidates the quota is reached before the pair splits

    def condition(s):
        assert g.box(0)[5] == 4
        assert expected_paths(s, 3)[3] == 2 and set(np.delete(expected_paths(s, 3), 3)) == {1}
        assert plan_depth(g, 3, 1) == 0 and set(expected_paths(s, 1)) == {2}
    return sc.Scene("kitti", g, pts, condition)


BUILDERS = {
    "cap_exact-3": lambda: scene_cap(320, 240, 500, 3, False),
    "cap_plus_one-3": lambda: scene_cap(320, 240, 500, 3, True),
    "cap_exact-tall-3": lambda: scene_cap(96, 320, 100, 3, False),
    "cap_plus_one-tall-3": lambda: scene_cap(96, 320, 100, 3, True),
    "mixed": scene_mixed,
    "boundaries-3": lambda: scene_boundaries(320, 240, 3),
    "boundaries-tall-3": lambda: scene_boundaries(96, 320, 3),
    "root_edges-4": lambda: scene_root_edges(620, 188, 4),
    "root_edges-5": lambda: scene_root_edges(632, 152, 5),
    "kitti": scene_kitti,
}
# scenes of octree_scenes that the issue's list names: both phase-1 exits, and phase 2's sequence tie-break
# with an early break; all of them must stay on the pyramid path
REUSED = ["phase1-N", "pair-stuck", "ties", "phase2-stuck"]
# pairs one pixel apart that phase 2 walks down: the rounds leave the pyramid path from PHASE 2
PHASE2_FALLBACK = "phase2-multi"
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def by_name(name):
    return BUILDERS[name]() if name in BUILDERS else sc.by_name(name)


def batch_of(name):
    """Three scenes of one geometry with `name` in the middle, fillers around it."""
    s = by_name(name)
    return [sc.filler_for(s.g.key, 0), s, sc.filler_for(s.g.key, 1)]

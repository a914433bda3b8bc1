"""k_octree's count-pyramid path on the CPU: the numpy model of it (tests/octree_pyramid_model.py) against
the literal DistributeOctTree (tests/octree_literal.py) for every pyramid depth, the bench's own scenes
against the plan's depth, the new scenes' path conditions, and the plan item ORBX_LP_OCT_PYRAMID.
tests/test_gpu_octree_pyramid.py holds the kernel to the literal's outputs and the model's paths."""
import functools

import numpy as np
import pytest

import oracle
import octree_pyramid_model as model
import octree_pyramid_scenes as ps
import octree_scenes as sc
from orb_slam2_commit_amd import synth

DEPTHS = range(model.MAX_DEPTH + 1)


def assert_model_is_literal(g, l, pts, lit_result, what):
    """For D = 0..6: the model's selection is the literal's, whichever path it took."""
    got = {}
    for D in DEPTHS:
        idx, path, deepest = ps.model_level(g, l, pts, D)
        assert np.array_equal(idx, lit_result["index"]), (what, "level", l, "D", D, path)
        assert (path == 0) == (len(pts) == 0)
        if len(pts):
            assert path == 2 if D == 0 else path in (1, 2)
            if path == 1:
                assert deepest < D
        got[D] = (path, deepest)
    # the deepest node split does not depend on D, and the path is 1 exactly from that depth + 1 on
    deep = got[model.MAX_DEPTH][1] if got[model.MAX_DEPTH][0] == 1 else None
    if len(pts) and deep is not None:
        for D in DEPTHS:
            assert got[D][0] == (1 if D > deep and D > 0 else 2), (what, l, got)
    return got


@pytest.mark.parametrize("name", sc.NAMES)
def test_model_is_the_literal_on_the_octree_scenes(name):
    s = sc.by_name(name)
    for l in range(s.g.nlevels):
        assert_model_is_literal(s.g, l, s.ordered[l], s.literal[l], name)


@pytest.mark.parametrize("name", ps.NAMES)
def test_model_is_the_literal_on_the_pyramid_scenes(name):
    s = ps.by_name(name)
    for l in range(s.g.nlevels):
        assert_model_is_literal(s.g, l, s.ordered[l], s.literal[l], name)


@pytest.mark.parametrize("name", ps.NAMES)
def test_scene_takes_the_path_it_is_named_for(name):
    s = ps.by_name(name)
    s.condition(s)


@pytest.mark.parametrize("name", ps.REUSED)
def test_reused_scenes_stay_on_the_pyramid_path(name):
    """Both phase-1 exits ('N'; 'stuck' with a node that still holds several points) and phase 2 with its
    tie-break, its early break and its 'stuck' exit."""
    s = sc.by_name(name)
    s.condition(s)
    p = ps.expected_paths(s, 3)
    assert set(p[[len(s.ordered[l]) > 0 for l in range(s.g.nlevels)]]) == {1}, (name, p)


@functools.lru_cache(maxsize=None)
def image_levels(w, h, nf, seed, right, stress):
    img = synth.stereo_pair(seed, w, h, stress=stress)[1 if right else 0]
    g = sc.geom(w, h, (nf,) + sc.P8)
    ref = oracle.extract(oracle.params(*g.params), img)
    return g, g.assemble(sc.fast_points(g, [ref.level(l) for l in range(g.nlevels)]))[2]


@pytest.mark.parametrize("case", [(640, 480, 1000, 3, False, False), (320, 240, 500, 4, False, False),
                                  (640, 480, 1000, 10, False, True)])
def test_model_is_the_literal_on_image_candidates(case):
    g, ordered = image_levels(*case)
    for l in range(g.nlevels):
        assert_model_is_literal(g, l, ordered[l], sc.literal_level(g, l, ordered[l]), case)


BENCH = [(s, right) for s in synth.sequence_seeds(0, 16)[:6] for right in (False,)] + \
        [(s, True) for s in synth.sequence_seeds(0, 16)[6:8]]


@pytest.mark.parametrize("seed,right", BENCH)
def test_bench_scenes_stay_on_the_pyramid_path(seed, right):
    """The benchmark's images (KITTI shape and parameters): every level stays on the pyramid path at the depth
    of its launch group (the benchmark's batches), with the literal's selection."""
    g, ordered = image_levels(1241, 376, 2000, seed, right, False)
    for l in range(g.nlevels):
        r = sc.literal_level(g, l, ordered[l])
        D = ps.plan_depth(g, l, 3)
        idx, path, deepest = ps.model_level(g, l, ordered[l], D)
        print("seed", seed, "right", right, "level", l, "T", len(ordered[l]), "D", D, "path", path, "deepest split", deepest)
        assert path == 1 and np.array_equal(idx, r["index"]), (seed, l, D, path, deepest)


def test_plan_item():
    """ORBX_LP_OCT_PYRAMID follows ORBX_LP_OCTREE's rows; the pyramid path fits the LDS the launch had without
    it."""
    for w, h, nf, P in [(1241, 376, 2000, sc.P8), (752, 480, 1200, sc.P8), (640, 480, 1000, sc.P8), (320, 240, 500, sc.P8),
                        (96, 320, 100, sc.P1), (632, 152, 1500, sc.P1)]:
        g = sc.geom(w, h, (nf,) + P)
        rows = ps.pyramid_rows(g)
        assert len(rows) == len(g.groups)
        for r, q in zip(rows, g.groups):
            D, nini, counters, nbytes, pyr_lds, gen_lds, lds, dmax = (int(v) for v in r)
            assert nini == max(g.box(l)[5] for l in range(int(q[0]), int(q[1])))
            assert pyr_lds <= gen_lds == lds == q[6]
            if q[7] >= 1:  # the one-launch row: the generic path alone
                assert (D, counters, nbytes, pyr_lds) == (0, 0, 0, 0)
                continue
            assert dmax == model.MAX_DEPTH and 1 <= D <= dmax
            assert counters == model.pyramid_counters(nini, D) and nbytes == (counters + 1) // 2 * 4
    g = sc.geom(1241, 376, (2000,) + sc.P8)
    # the 512-thread group holds depth 5 beside its candidates; the 256-thread group, whose blocks have
    # half the LDS, depth 4; the one-launch row none.  The bench's levels split nodes of depth 3 at the
    # deepest (test_bench_scenes_stay_on_the_pyramid_path)
    assert [int(r[0]) for r in ps.pyramid_rows(g)] == [5, 4, 0]
    assert int(ps.pyramid_rows(g)[0][2]) == 5460


def test_phase2_fallback_scene():
    """phase2-multi leaves the pyramid path from a phase-2 round."""
    s = sc.by_name(ps.PHASE2_FALLBACK)
    s.condition(s)
    D = ps.plan_depth(s.g, 0, 3)
    assert D >= 4 and ps.model_level(s.g, 0, s.ordered[0], D)[1] == 2
    assert [e["phase"] for e in s.literal[0]["trace"]].count(1) <= 3  # phase 1 ends at depth <= 3

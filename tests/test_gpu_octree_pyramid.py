"""k_octree's two paths through orbx_debug_octree_paths: every output is the literal's
(tests/octree_literal.py), and the path each (image, level) block reports is the model's
(tests/octree_pyramid_model.py) at the depth D of the launch row it ran under (ORBX_LP_OCT_PYRAMID).
Batches of one image (the one-launch row, whose D is 0: the generic path alone) and of three (the launch
groups).  Scenes: tests/octree_pyramid_scenes.py (tests/test_octree_pyramid.py proves their path
conditions on the CPU).

depth_zero: the one-launch row is a plan row whose D is 0, so every one-image test runs it.  For the
launch groups, whose D is never 0 (the pyramid path needs less LDS than the generic path at every node
capacity), the test uses the entry's depth_cap argument, a call-time cap: depth_cap = 0 launches the
groups with D = 0, which never enter the pyramid path -- the previous kernel body alone."""
import numpy as np
import pytest

import octree_pyramid_scenes as ps
import octree_scenes as sc
from orb_slam2_commit_amd import ORBextractor
from orb_slam2_commit_amd.orb import debug_octree_paths

pytestmark = pytest.mark.gpu

_handles = {}


def handle(g):
    if g.key not in _handles:
        ex = ORBextractor(*g.params)
        ex(np.full((g.h, g.w), 128, np.uint8))
        _handles[g.key] = ex
    return _handles[g.key]


def run(batch, depth_cap=-1):
    g = batch[0].g
    cnt, out, paths = debug_octree_paths(handle(g), np.stack([b.counts for b in batch]), np.stack([b.cand for b in batch]),
                                         depth_cap)
    for i, b in enumerate(batch):
        exp_cnt, exp_out = b.expected()
        what = (b.name, "image", i, "of", len(batch), "cap", depth_cap)
        for l in range(g.nlevels):
            off, cap = int(g.levels[l][6]), int(g.levels[l][7])
            assert cnt[i][l] == exp_cnt[l], (what, "level", l, "count", int(cnt[i][l]), int(exp_cnt[l]))
            assert np.array_equal(out[i][off:off + cap], exp_out[off:off + cap]), (what, "level", l)
        exp_paths = ps.expected_paths(b, len(batch), depth_cap)
        assert np.array_equal(paths[i], exp_paths), (what, "paths", paths[i].tolist(), exp_paths.tolist())
    return paths


@pytest.mark.parametrize("name", ps.NAMES + ps.REUSED + [ps.PHASE2_FALLBACK])
def test_scene_one_image(gpu, name):
    run([ps.by_name(name)])


@pytest.mark.parametrize("name", ps.NAMES + ps.REUSED + [ps.PHASE2_FALLBACK])
def test_scene_in_a_batch_of_three(gpu, name):
    run(ps.batch_of(name))


def test_mixed_paths_differ_per_block(gpu):
    """One launch: a block that leaves the pyramid path beside blocks that stay and an empty level."""
    paths = run(ps.batch_of("mixed"))
    assert {0, 1, 2} <= set(paths[1].tolist()), paths
    assert set(run([ps.by_name("mixed")]).ravel().tolist()) == {0, 2}


@pytest.mark.parametrize("name", ["mixed", "kitti", "cap_exact-3", "root_edges-5", "ties", "bitonic-tail", "kcap-g1+1"])
def test_depth_zero_is_the_generic_path_alone(gpu, name):
    for batch in ([ps.by_name(name)], ps.batch_of(name)):
        paths = run(batch, depth_cap=0)
        assert 1 not in set(paths.ravel().tolist())


@pytest.mark.parametrize("cap", [1, 2, 3, 4, 5])
def test_every_depth_below_the_plans(gpu, cap):
    """The same launches at D = min(plan's, cap): shallower pyramids leave the path earlier, with the same outputs."""
    for name in ("kitti", "boundaries-3", "phase2-multi"):
        run(ps.batch_of(name), depth_cap=cap)

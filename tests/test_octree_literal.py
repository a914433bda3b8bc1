"""DistributeOctTree three ways on the CPU: the literal restatement (tests/octree_literal.py) against the
C++ oracle's distribute_octree, on crafted candidate sets that take one path each
(tests/octree_scenes.py) and on the true FAST candidates of images; every scene's path condition; and
the host check that guards k_octree's injection entry point.  tests/test_gpu_octree.py holds the kernel
to the same literal.  Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import octree_literal as lit
import octree_scenes as sc
from orb_slam2_commit_amd import _lib, synth

IMAGES = [("tum", 3, 640, 480, 1000, False), ("small", 4, 320, 240, 500, False), ("noise", 10, 640, 480, 1000, True)]


def oracle_level(g, l, pts):
    minBX, minBY, maxBX, maxBY, N, _ = g.box(l)
    return oracle.distribute_octree(pts[:, 0] - minBX, pts[:, 1] - minBY, pts[:, 2], minBX, maxBX, minBY, maxBY, N)


def check(g, counts, cand, n_img=1):
    p = _lib.ExtractorParams(*g.params)
    counts = np.ascontiguousarray(counts, np.int32)
    cand = np.ascontiguousarray(cand, np.uint32)
    return _lib.lib().orbx_debug_octree_candidates_check(C.byref(p), g.w, g.h, n_img, _lib.ptr(counts), _lib.ptr(cand))


@pytest.mark.parametrize("name", sc.NAMES)
def test_scene_takes_the_path_it_is_named_for(name):
    s = sc.by_name(name)
    s.condition(s)


@pytest.mark.parametrize("name", sc.NAMES)
def test_literal_pins_the_oracle_on_scene(name):
    s = sc.by_name(name)
    for l in range(s.g.nlevels):
        got = oracle_level(s.g, l, s.ordered[l])
        assert np.array_equal(got, s.literal[l]["index"]), (name, l, s.literal[l]["trace"])


def test_scenes_cover_every_round_exit():
    """Over the scene set: both loops end by 'N' and by 'stuck', phase 1 continues and switches, phase 2
    continues, breaks mid-list and runs a vector to its end; roots are erased; nIni is 1, 4 and 5."""
    seen, n_ini, erased = set(), set(), 0
    for name in sc.NAMES:
        for r in sc.by_name(name).literal:
            seen |= {(e["phase"], e["exit"], e["broke"]) for e in r["trace"]}
            if r["trace"]:
                n_ini.add(r["nIni"])
            erased += r["roots_erased"]
    assert seen >= {(1, "N", False), (1, "stuck", False), (1, "next", False), (1, "phase2", False), (2, "N", True),
                    (2, "stuck", False), (2, "next", False)}, seen
    assert n_ini >= {1, 4, 5} and erased >= 4


@functools.lru_cache(maxsize=None)
def image_case(name):
    _, seed, w, h, nf, stress = next(c for c in IMAGES if c[0] == name)
    img = synth.stereo_pair(seed, w, h, stress=stress)[0]
    g = sc.geom(w, h, (nf,) + sc.P8)
    ref = oracle.extract(oracle.params(*g.params), img)
    counts, cand, ordered = g.assemble(sc.fast_points(g, [ref.level(l) for l in range(g.nlevels)]))
    return g, ref, counts, cand, ordered


@pytest.mark.parametrize("name", [c[0] for c in IMAGES])
def test_literal_pins_the_oracle_on_image_candidates(name):
    """All levels: the literal's selection is distribute_octree's, and it is what oracle.extract kept:
    the keypoints' (x, y) are the selected pixels times the level's scale, with their response and octave."""
    g, ref, counts, cand, ordered = image_case(name)
    assert check(g, counts, cand) == 0
    scale = oracle.scale_tables(oracle.params(*g.params))["scale"]
    kp = ref.keypoints
    for l in range(g.nlevels):
        r = sc.literal_level(g, l, ordered[l])
        assert np.array_equal(oracle_level(g, l, ordered[l]), r["index"]), (name, l)
        sel = ordered[l][r["index"]]
        k = kp[kp["octave"] == l]
        assert len(k) == len(sel) > 0, (name, l)
        sx = sel[:, 0].astype(np.float32) * (scale[l] if l else np.float32(1))
        sy = sel[:, 1].astype(np.float32) * (scale[l] if l else np.float32(1))
        assert np.array_equal(k["x"].view(np.uint32), sx.view(np.uint32)), (name, l)
        assert np.array_equal(k["y"].view(np.uint32), sy.view(np.uint32)), (name, l)
        assert np.array_equal(k["response"], sel[:, 2].astype(np.float32)), (name, l)


def test_noise_image_overflows_the_rank_sort_nowhere_but_spills():
    """What the 640x480 noise image does and does not reach (the GPU tests choose their cases by it): its
    level 0 holds more candidates than the one-launch row keeps in LDS, and no level reaches the bitonic
    sort, which is why tests/test_gpu_octree.py brings a one-level extractor with a large quota."""
    g, _, _, _, ordered = image_case("noise")
    assert len(ordered[0]) > g.groups[-1][5]
    for l in range(g.nlevels):
        r = sc.literal_level(g, l, ordered[l])
        assert max(e["M"] for e in r["trace"] if e["phase"] == 2) <= sc.RANK_SORT_MAX


# ------------------------------------------------------------------ the injection entry's host check
@pytest.mark.parametrize("name", sc.NAMES)
def test_check_accepts_scene(name):
    s = sc.by_name(name)
    assert check(s.g, s.counts, s.cand) == 0
    batch, _ = sc.batch_of(name)
    assert len({b.name for b in batch}) == 3 and all(b.g.key == s.g.key for b in batch)
    assert check(s.g, np.stack([b.counts for b in batch]), np.stack([b.cand for b in batch]), 3) == 0


def test_check_refusals():
    s = sc.by_name("slots")
    g = s.g
    ci = int(np.flatnonzero(s.counts > 0)[0])
    off, cap = int(g.cells[ci][5]), int(g.cells[ci][6])
    l = int(g.cells[ci][0])
    minBX, minBY, maxBX, maxBY = g.box(l)[:4]
    assert check(g, s.counts, s.cand) == 0

    def with_cand(v):
        c = s.cand.copy()
        c[off] = v
        return check(g, s.counts, c)

    def pack(x, y):
        return (9 << 24) | (y << 12) | x
    y0 = int((s.cand[off] >> 12) & 0xFFF)
    over = s.counts.copy()
    over[ci] = cap + 1
    assert check(g, over, s.cand) == -1  # a count above cap
    under = s.counts.copy()
    under[ci] = -1
    assert check(g, under, s.cand) == -1
    assert with_cand(pack(maxBX - 1, y0)) == 0 and with_cand(pack(maxBX, y0)) == -1  # a point on maxBX
    assert with_cand(pack(minBX, minBY)) == 0 and with_cand(pack(minBX - 1, minBY)) == -1
    assert with_cand(pack(minBX, maxBY)) == -1 and with_cand(pack(minBX, minBY - 1)) == -1
    assert with_cand(int(s.cand[off + 1]) & 0xFFFFFF) == -1  # a duplicate pixel (another score)
    # the same pixel on two levels, or in two images, is no duplicate
    two = np.stack([s.counts, s.counts]), np.stack([s.cand, s.cand])
    assert check(g, two[0], two[1], 2) == 0
    assert check(g, s.counts, s.cand, 0) == -1 and check(g, two[0], two[1], 65) == -1
    assert _lib.lib().orbx_debug_octree_candidates_check(None, g.w, g.h, 1, _lib.ptr(s.counts), _lib.ptr(s.cand)) == -1
    p = _lib.ExtractorParams(*g.params)
    assert _lib.lib().orbx_debug_octree_candidates_check(C.byref(p), g.w, g.h, 1, None, _lib.ptr(s.cand)) == -1


def test_literal_root_guard():
    """96x320: the root count rounds to 0 in the reference (deviation 2); the plan and the literal clamp."""
    g = sc.geom(96, 320, (100,) + sc.P1)
    minBX, minBY, maxBX, maxBY, _, n_ini = g.box(0)
    assert lit.root_count(minBX, maxBX, minBY, maxBY)[:2] == (0, 1) and n_ini == 1

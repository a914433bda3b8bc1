"""k_resize_strip (the fast path of a pyramid level) and the plan's choice between it and k_resize.

Every pyramid level is compared bit for bit with oracle.extract(...).level(l).  The strip kernel's
output tile is 256 x 32 (four strips of 8 rows); the sizes below put level 1 one column over and
exactly at a tile multiple, one row over and exactly at a strip and a tile multiple, and make a
level a single partial tile; their level widths cover every residue mod 4 (the dword store against
the byte stores of a row's last columns).  The CPU part reads the path per level from
orbx_debug_launch_plan (ORBX_LP_PATH): the strip kernel on levels 1-7 of the KITTI, EuRoC and TUM
geometries at 1.2, k_resize where a large scale factor's footprint does not fit the strip kernel.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from orb_slam2_commit_amd import _lib

LEVELS, PATH = 1, 8
NL, INI, MIN = 8, 20, 7
RS_TW, RS_TH, RS_R = 256, 32, 8

# name -> (w, h, nfeatures, scale factor)
SHAPES = {
    "w257_h33": (308, 40, 300, 1.2),   # level 1 = 257 x 33: one column / one row over a tile
    "w256_h32": (307, 38, 300, 1.2),   # level 1 = 256 x 32: exactly one tile
    "h41": (203, 49, 300, 1.2),        # level 1 = 169 x 41: one row over a strip multiple
    "h40": (202, 48, 300, 1.2),        # level 1 = 168 x 40: a strip multiple
    "partial": (64, 48, 300, 1.2),     # levels 3.. a single partial tile each
    "two_tiles": (333, 85, 300, 1.2),  # level 1 = 278 x 71: 2 x 3 tiles, partial in both directions
    "smallest": (2, 2, 300, 1.2),      # the smallest image the plan accepts (1 x 1 is refused)
    "sf1.1": (320, 240, 500, 1.1),     # another scale factor on the fast path
    "sf1.5": (320, 240, 500, 1.5),     # accepted, levels 1-5 on k_resize (the footprint rows do not fit)
}


def plan(what, w, h, nf, sf):
    L = _lib.lib()
    p = _lib.ExtractorParams(nf, sf, NL, INI, MIN)
    n = L.orbx_debug_launch_plan(C.byref(p), w, h, what, 0, 0, 0, None, 0)
    if n < 0:
        return n
    out = np.zeros(n, np.int64)
    assert L.orbx_debug_launch_plan(C.byref(p), w, h, what, 0, 0, 0, _lib.ptr(out), n) == n
    return out.reshape(-1, 8)


def level_dims(name):
    w, h, nf, sf = SHAPES[name]
    return [tuple(int(v) for v in r[:2]) for r in plan(LEVELS, w, h, nf, sf)]


# ------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name,w,h,nf", [("kitti", 1241, 376, 2000), ("euroc", 752, 480, 1200), ("tum", 640, 480, 1000)])
def test_fast_path_on_every_level_at_1_2(name, w, h, nf):
    path = plan(PATH, w, h, nf, 1.2)
    dims = [tuple(r[:2]) for r in plan(LEVELS, w, h, nf, 1.2)]
    assert len(path) == NL - 1
    for l in range(1, NL):
        f, gx, gy, tw, th, stride, rows, r = (int(v) for v in path[l - 1])
        assert (f, tw, th, r) == (1, RS_TW, RS_TH, RS_R), (l, path[l - 1])
        assert (gx, gy) == (-(-dims[l][0] // tw), -(-dims[l][1] // th))
        assert stride % 16 == 0 and stride >= 16 and rows >= 1


def test_general_path_for_a_large_scale_factor():
    w, h, nf, sf = SHAPES["sf1.5"]
    path = plan(PATH, w, h, nf, sf)
    dims = [tuple(r[:2]) for r in plan(LEVELS, w, h, nf, sf)]
    # 32 output rows x 1.5 need 49 source rows, more than the strip kernel stages: levels taller than
    # one strip tile keep k_resize (128 x 32 tiles), the last two fit the strip kernel
    assert [int(r[0]) for r in path] == [0, 0, 0, 0, 0, 1, 1]
    for l in range(1, 6):
        f, gx, gy, tw, th, stride, rows, r = (int(v) for v in path[l - 1])
        assert (tw, th, r) == (128, 32, 0) and (gx, gy) == (-(-dims[l][0] // 128), -(-dims[l][1] // 32))
    # and 1.1 stays on the fast path
    w, h, nf, sf = SHAPES["sf1.1"]
    assert [int(r[0]) for r in plan(PATH, w, h, nf, sf)] == [1] * 7


def test_shapes_are_what_they_claim():
    assert level_dims("w257_h33")[1] == (RS_TW + 1, RS_TH + 1)
    assert level_dims("w256_h32")[1] == (RS_TW, RS_TH)
    assert level_dims("h41")[1][1] == 5 * RS_R + 1 and level_dims("h40")[1][1] == 5 * RS_R
    assert all(w <= RS_TW and h <= RS_TH for w, h in level_dims("partial")[3:])
    assert level_dims("two_tiles")[1] == (278, 71)
    widths = {w % 4 for n in SHAPES if SHAPES[n][3] == 1.2 for w, _ in level_dims(n)[1:]}
    assert widths == {0, 1, 2, 3}
    # 2 x 2 is the smallest image: 1 x 1 has an empty last level
    assert isinstance(plan(LEVELS, 1, 1, 300, 1.2), int) and plan(LEVELS, 1, 1, 300, 1.2) < 0
    assert not isinstance(plan(LEVELS, 2, 2, 300, 1.2), int)
    # every 1.2 shape here runs the strip kernel on its levels of more than one row and column
    for n in ("w257_h33", "w256_h32", "h41", "h40", "partial", "two_tiles"):
        w, h, nf, sf = SHAPES[n]
        assert [int(r[0]) for r in plan(PATH, w, h, nf, sf)] == [1] * 7, n


# ------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _reference(name, seed):
    """Image `seed` of a shape and the oracle's pyramid of it, computed once."""
    import oracle
    from orb_slam2_commit_amd import synth
    w, h, nf, sf = SHAPES[name]
    if min(w, h) >= 32:
        img = synth.stereo_pair(seed, w, h)[0]
    else:
        img = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    ref = oracle.extract(oracle.params(nf, sf, NL, INI, MIN), img)
    return img, [ref.level(l) for l in range(NL)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_pyramid_levels_bitexact(gpu, name):
    from orb_slam2_commit_amd import ORBextractor
    w, h, nf, sf = SHAPES[name]
    img, levels = _reference(name, 11)
    ex = ORBextractor(nf, sf, NL, INI, MIN)
    ex(img)
    for l in range(NL):
        got = ex.pyramid_level(l)
        assert got.shape == levels[l].shape, (l, got.shape)
        assert np.array_equal(got, levels[l]), "pyramid level %d differs" % l


@pytest.mark.gpu
def test_batch_of_three_images(gpu):
    """Three different images in one extract_batch_device call: the per-image addressing of the input
    (level 1 reads the input batch at its pitch) and of the pyramid block (levels 2.. read level l - 1)."""
    import torch
    from orb_slam2_commit_amd import ORBextractor
    name = "two_tiles"
    w, h, nf, sf = SHAPES[name]
    refs = [_reference(name, 11 + i) for i in range(3)]
    assert not np.array_equal(refs[0][0], refs[1][0]) and not np.array_equal(refs[1][0], refs[2][0])
    ex = ORBextractor(nf, sf, NL, INI, MIN)
    cap = ex.max_keypoints(w, h)
    d_img = torch.from_numpy(np.stack([r[0] for r in refs])).to(gpu)
    kps = torch.zeros((3, cap, 28), dtype=torch.uint8, device=gpu)
    desc = torch.zeros((3, cap, 32), dtype=torch.uint8, device=gpu)
    cnt = torch.zeros(3, dtype=torch.int32, device=gpu)
    ex.extract_batch_device(d_img, kps, desc, cnt, torch.cuda.current_stream())
    torch.cuda.synchronize()
    for i, (_, levels) in enumerate(refs):
        for l in range(NL):
            assert np.array_equal(ex.pyramid_level(l, i), levels[l]), (i, l)

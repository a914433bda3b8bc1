"""k_describe's patch slot table and the gather it drives, bit-exact against the oracle.

The table maps load slot s = lane + 64 * load to (patch row, k-th 16-B chunk of the row's span).  Its
order is free as far as the result goes (address, validity and LDS destination are functions of
(row, chunk)), so the table is checked as a set against the rule it restates and for the quad
structure the gather relies on; the extraction runs on images whose oracle keypoints put the patch
origin at every alignment inside a 16-B chunk and every row phase inside an 8-row tile.
"""
import numpy as np
import pytest

import oracle
from orb_slam2_commit_amd import ORBextractor, synth
from orb_slam2_commit_amd import _lib

pytestmark = pytest.mark.gpu

DBG_PATCH_SLOTS = 8
PATCH_R = 18
# c_patch_hw: the half-width of patch row r the rotated pattern can reach
PATCH_HW = [6, 8, 10, 11, 12, 13, 14, 15, 16, 16, 17, 17, 18, 18, 18, 18, 18, 18, 18,
            18, 18, 18, 18, 18, 18, 17, 17, 16, 16, 15, 14, 13, 12, 11, 10, 8, 6]
# 320 x 240 images (synth.stereo_pair's left image) chosen on the CPU from the oracle's keypoints alone
SEEDS = [114, 97, 91, 0]
W, H, NF = 320, 240, 500


def _row_chunks(r):
    """The most 16-B chunks the span [18 + a - hw, 18 + a + hw] of row r covers over a = 0..15."""
    hw = PATCH_HW[r]
    return max(((PATCH_R + a + hw) >> 4) - ((PATCH_R + a - hw) >> 4) + 1 for a in range(16))


def _slot_table(ex):
    L = _lib.lib()
    n = L.orbx_debug_copy(ex._h, DBG_PATCH_SLOTS, 0, 0, None, 0)
    assert n == 128 * 4, n
    buf = np.zeros(n, np.uint8)
    L.orbx_debug_copy(ex._h, DBG_PATCH_SLOTS, 0, 0, _lib.ptr(buf), n)
    return buf.view(np.int32)


def test_slot_table(gpu):
    ex = ORBextractor(NF, 1.2, 8, 20, 7)
    ex(synth.stereo_pair(SEEDS[0], W, H)[0])  # the debug copy reads a handle that has extracted
    tab = _slot_table(ex)
    assert len(tab) == 128
    used = [int(e) for e in tab if e != 0xFF]
    per_row = [_row_chunks(r) for r in range(2 * PATCH_R + 1)]
    assert sorted(set(per_row)) == [2, 3, 4]
    expect = sorted((r << 2) | k for r in range(2 * PATCH_R + 1) for k in range(per_row[r]))
    assert len(expect) == 124
    assert len(used) <= 128 and sorted(used) == expect, "not the 124 (row, chunk) slots, each once"
    # the four lanes of a quad: one chunk index, consecutive rows -- all quads but at most one
    odd = 0
    for q in range(32):
        ent = [int(e) for e in tab[4 * q:4 * q + 4] if e != 0xFF]
        if not ent:
            continue
        rows, chunks = [e >> 2 for e in ent], [e & 3 for e in ent]
        if not (len(ent) == 4 and len(set(chunks)) == 1 and rows == list(range(rows[0], rows[0] + 4))):
            odd += 1
    assert odd <= 1, "%d quads are not four consecutive rows of one chunk index" % odd


def _phases(p, ref):
    """(x - 18) & 15, (y - 18) & 7 and the level of every oracle keypoint, in level coordinates."""
    sc = oracle.scale_tables(p)["scale"]
    k = ref.keypoints
    lv = k["octave"].astype(int)
    x = np.rint(k["x"] / sc[lv]).astype(int)
    y = np.rint(k["y"] / sc[lv]).astype(int)
    return (x - PATCH_R) & 15, (y - PATCH_R) & 7, lv


def test_extract_every_patch_phase(gpu):
    p = oracle.params(NF, 1.2, 8, 20, 7)
    ex = ORBextractor(NF, 1.2, 8, 20, 7)
    seen0, seen1 = set(), set()
    for seed in SEEDS:
        img = synth.stereo_pair(seed, W, H)[0]
        ref = oracle.extract(p, img)
        kps, desc = ex(img)
        assert len(kps) == len(ref.keypoints)
        assert np.array_equal(kps.view(np.uint8), ref.keypoints.view(np.uint8)), "keypoints differ (seed %d)" % seed
        assert np.array_equal(desc, ref.descriptors), "descriptors differ (seed %d)" % seed
        a, b, lv = _phases(p, ref)
        seen0 |= set(zip(a[lv == 0].tolist(), b[lv == 0].tolist()))
        seen1 |= set(zip(a[lv >= 1].tolist(), b[lv >= 1].tolist()))
    every = {(a, b) for a in range(16) for b in range(8)}
    assert seen0 == every, "level 0 misses %s" % sorted(every - seen0)
    assert seen1 == every, "levels >= 1 miss %s" % sorted(every - seen1)

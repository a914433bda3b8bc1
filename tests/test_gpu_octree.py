"""k_octree against the literal restatement of DistributeOctTree (tests/octree_literal.py), exactly.

Scenes (tests/octree_scenes.py, one per path; tests/test_octree_literal.py proves on the CPU that each
takes its path and that the literal is the oracle's distribute_octree) go through
orbx_debug_octree_candidates, which stages supplied candidates and runs the shipped launch path: one
launch over every level for one image, the 512- and 256-thread launch groups for three.  On real
extractions the kernel's own input (ORBX_DBG_CANDIDATES) is fed to the literal, which localises a
mismatch to this stage, and whole extractions that reach the bitonic sort, the groups' spill path, the
root-count guard and tiny quotas are compared with oracle.extract bit for bit."""
import numpy as np
import pytest

import oracle
import octree_scenes as sc
from orb_slam2_commit_amd import ORBextractor, _lib, synth
from orb_slam2_commit_amd.orb import debug_octree_candidates

pytestmark = pytest.mark.gpu

DBG_CELL_COUNTS, DBG_CAND, DBG_OCT_COUNTS, DBG_OCT_OUT = 2, 4, 5, 6
_handles = {}


def handle(g):
    """An extractor whose last call was an extraction on g's geometry (a flat image: no keypoints)."""
    if g.key not in _handles:
        ex = ORBextractor(*g.params)
        ex(np.full((g.h, g.w), 128, np.uint8))
        _handles[g.key] = ex
    return _handles[g.key]


def dbg(ex, what, image=0, dtype=np.int32):
    L = _lib.lib()
    n = L.orbx_debug_copy(ex._h, what, image, 0, None, 0)
    assert n >= 0, n
    buf = np.zeros(max(n, 1), np.uint8)
    L.orbx_debug_copy(ex._h, what, image, 0, _lib.ptr(buf), n)
    return buf[:n].view(dtype)


def assert_levels(g, got_cnt, got_out, exp_cnt, exp_out, what):
    """Counts, the first count slots and the untouched rest, level by level."""
    for l in range(g.nlevels):
        off, cap = int(g.levels[l][6]), int(g.levels[l][7])
        assert got_cnt[l] == exp_cnt[l], (what, "level", l, "count", int(got_cnt[l]), int(exp_cnt[l]))
        a, b = got_out[off:off + cap], exp_out[off:off + cap]
        assert np.array_equal(a, b), (what, "level", l, "slots", np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


@pytest.mark.parametrize("name", sc.NAMES)
def test_scene_one_image(gpu, name):
    s = sc.by_name(name)
    cnt, out = debug_octree_candidates(handle(s.g), s.counts[None], s.cand[None])
    assert_levels(s.g, cnt[0], out[0], *s.expected(), what=name)


@pytest.mark.parametrize("name", sc.NAMES)
def test_scene_in_a_batch_of_three(gpu, name):
    """The launch groups; three different scenes, so an index that crosses images shows."""
    batch, at = sc.batch_of(name)
    assert batch[at].name == name and len({b.name for b in batch}) == 3
    g = batch[at].g
    cnt, out = debug_octree_candidates(handle(g), np.stack([b.counts for b in batch]), np.stack([b.cand for b in batch]))
    for i, b in enumerate(batch):
        assert_levels(g, cnt[i], out[i], *b.expected(), what=(name, "image", i, b.name))


def test_injection_leaves_the_extraction_alone_and_checks_first(gpu):
    """The handle's stage buffers survive an injection, and a bad input is refused before any launch."""
    g = sc.geom(320, 240, (500,) + sc.P8)
    ex = ORBextractor(*g.params)
    img = synth.stereo_pair(4, 320, 240)[0]
    kps, desc = ex(img)
    before = [dbg(ex, w).copy() for w in (DBG_CELL_COUNTS, DBG_CAND, DBG_OCT_COUNTS, DBG_OCT_OUT)]
    s = sc.by_name("few")
    cnt, out = debug_octree_candidates(ex, s.counts[None], s.cand[None])
    assert_levels(g, cnt[0], out[0], *s.expected(), what="few")
    for w, b in zip((DBG_CELL_COUNTS, DBG_CAND, DBG_OCT_COUNTS, DBG_OCT_OUT), before):
        assert np.array_equal(dbg(ex, w), b), w
    over = s.counts.copy()
    over[int(np.flatnonzero(over)[0])] = 10000
    with pytest.raises(_lib.OrbxError) as e:
        debug_octree_candidates(ex, over[None], s.cand[None])
    assert e.value.code == _lib.ORBX_ERR_ARG
    fresh = ORBextractor(*g.params)
    fresh._last_shape = (320, 240)
    with pytest.raises(_lib.OrbxError) as e:
        debug_octree_candidates(fresh, s.counts[None], s.cand[None])
    assert e.value.code == _lib.ORBX_ERR_STATE


# ------------------------------------------------------------------ the stage on real extractions
def literal_of_device_candidates(ex, g, image=0):
    counts = dbg(ex, DBG_CELL_COUNTS, image)
    cand = dbg(ex, DBG_CAND, image, np.uint32)
    cnt = np.zeros(g.nlevels, np.int32)
    out = np.full(g.oct_total, sc.EMPTY, np.uint32)
    traces = []
    for l in range(g.nlevels):
        v = np.concatenate([cand[int(g.cells[ci][5]):int(g.cells[ci][5]) + counts[ci]] for ci in g.level_cells(l)] +
                           [np.zeros(0, np.uint32)]).astype(np.int64)
        pts = np.column_stack([v & 0xFFF, (v >> 12) & 0xFFF, v >> 24])
        r = sc.literal_level(g, l, pts)
        cnt[l] = len(r["packed"])
        off = int(g.levels[l][6])
        out[off:off + cnt[l]] = r["packed"]
        traces.append(r["trace"])
    return cnt, out, traces


@pytest.mark.parametrize("name,seed,w,h,nf,stress", [("kitti", 0, 1241, 376, 2000, False), ("euroc", 2, 752, 480, 1200, False),
                                                    ("noise", 10, 640, 480, 1000, True)])
def test_stage_on_real_candidates(gpu, name, seed, w, h, nf, stress):
    """After an extraction, the literal on the kernel's own input is the kernel's output."""
    g = sc.geom(w, h, (nf,) + sc.P8)
    ex = ORBextractor(*g.params)
    ex(synth.stereo_pair(seed, w, h, stress=stress)[0])
    cnt, out, _ = literal_of_device_candidates(ex, g)
    got_cnt, got_out = dbg(ex, DBG_OCT_COUNTS), dbg(ex, DBG_OCT_OUT, dtype=np.uint32)
    for l in range(g.nlevels):
        off = int(g.levels[l][6])
        assert got_cnt[l] == cnt[l], (name, l)
        assert np.array_equal(got_out[off:off + cnt[l]], out[off:off + cnt[l]]), (name, l)


# ------------------------------------------------------------------ end to end against oracle.extract
def rebuilt_candidates(g, img):
    ref = oracle.extract(oracle.params(*g.params), img)
    _, _, ordered = g.assemble(sc.fast_points(g, [ref.level(l) for l in range(g.nlevels)]))
    return ref, ordered


def assert_extraction(ex, img, ref, what):
    kps, desc = ex(img)
    assert len(kps) == len(ref.keypoints), (what, len(kps), len(ref.keypoints))
    assert kps.tobytes() == ref.keypoints.tobytes(), (what, "keypoints")
    assert np.array_equal(desc, ref.descriptors), (what, "descriptors")


def test_extract_reaches_the_bitonic_sort(gpu):
    """One level with a quota of 1500 on noise: phase 2 sorts more than 1024 splittable nodes, and the
    level's candidates overflow the one-launch row's LDS slots."""
    g = sc.geom(632, 152, (1500,) + sc.P1)
    img = synth.stereo_pair(40, 632, 152, stress=True)[0]
    ref, ordered = rebuilt_candidates(g, img)
    r = sc.literal_level(g, 0, ordered[0])
    M = max(e["M"] for e in r["trace"] if e["phase"] == 2)
    print("T", len(ordered[0]), "kcap", int(g.groups[-1][5]), "M", M)
    assert M > sc.RANK_SORT_MAX and len(ordered[0]) > g.groups[-1][5]
    assert_extraction(ORBextractor(*g.params), img, ref, "bitonic")


def test_batch_of_noise_spills_in_both_groups(gpu):
    import torch
    g = sc.geom(640, 480, (1000,) + sc.P8)
    imgs = [synth.stereo_pair(50 + i, 640, 480, stress=True)[0] for i in range(3)]
    refs = []
    for img in imgs:
        ref, ordered = rebuilt_candidates(g, img)
        refs.append(ref)
        T = [len(ordered[l]) for l in range(g.nlevels)]
        print("T", T, "groups", g.groups[:, [0, 1, 2, 5]].tolist())
        rows = g.groups[:-1]
        assert len(rows) == 2 and rows[0][2] == 512 and rows[1][2] == 256
        for row in rows:
            assert any(T[l] > row[5] for l in range(row[0], row[1])), (row, T)
        assert any(0 < T[l] < g.group_row(l, 3)[5] for l in range(g.nlevels))
    ex = ORBextractor(*g.params)
    cap = ex.max_keypoints(640, 480)
    kps = torch.zeros((3, cap, 28), dtype=torch.uint8, device=gpu)
    desc = torch.zeros((3, cap, 32), dtype=torch.uint8, device=gpu)
    cnt = torch.zeros(3, dtype=torch.int32, device=gpu)
    ex.extract_batch_device(torch.from_numpy(np.stack(imgs)).to(gpu), kps, desc, cnt, torch.cuda.current_stream())
    torch.cuda.synchronize()
    cnt, kps, desc = cnt.cpu().numpy(), kps.cpu().numpy(), desc.cpu().numpy()
    for i, ref in enumerate(refs):
        assert cnt[i] == len(ref.keypoints), i
        assert kps[i, :cnt[i]].tobytes() == ref.keypoints.tobytes(), (i, "keypoints")
        assert np.array_equal(desc[i, :cnt[i]], ref.descriptors), (i, "descriptors")


@pytest.mark.parametrize("stress", [False, True])
def test_extract_portrait_root_guard(gpu, stress):
    """96x320: (maxX - minX) / (maxY - minY) rounds to 0 roots; the oracle and the plan clamp to 1."""
    g = sc.geom(96, 320, (300,) + sc.P8)
    img = synth.stereo_pair(45, 96, 320, stress=stress)[0]
    ref, ordered = rebuilt_candidates(g, img)
    r = sc.literal_level(g, 0, ordered[0])
    assert r["nIni_raw"] == 0 and r["nIni"] == 1 and len(ordered[0]) > 1 and len(ref.keypoints) > 0
    assert_extraction(ORBextractor(*g.params), img, ref, "portrait")


def test_extract_tiny_quotas(gpu):
    """Quotas of 0-2 per level: every level finishes after its first round, and a level's output slots
    are the 4 * nIni the roots can make, not its quota + 3."""
    g = sc.geom(320, 240, (8,) + sc.P8)
    assert g.levels[:, 4].max() <= 2 and g.levels[:, 4].min() == 0
    assert all(int(c) == max(4 * int(n), int(q) + 3) for q, n, c in g.levels[:, [4, 5, 7]])
    assert any(4 * int(n) > int(q) + 3 for q, n, c in g.levels[:, [4, 5, 7]])
    img = synth.stereo_pair(4, 320, 240)[0]
    ref, ordered = rebuilt_candidates(g, img)
    for l in range(g.nlevels):
        r = sc.literal_level(g, l, ordered[l])
        assert len(r["trace"]) == 1 and r["trace"][0]["exit"] == "N", (l, r["trace"])
    assert_extraction(ORBextractor(*g.params), img, ref, "tiny quotas")

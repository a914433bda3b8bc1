"""k_resize's by-value launch descriptor, the division-free XCD block remap of the extraction and
stereo kernels, k_blur's swizzled write-out, and the addressing they introduce.

CPU part: orbx_debug_launch_plan builds the descriptors on the host exactly as an extractor handle
does (no device); every ResizeDesc field is recomputed here from the level sizes (the formulas of
bench.py:level_sizes), the footprint-bound tables are checked against the resize coefficient tables,
and the remap constants are checked exhaustively against // and %.  (k_blur and k_fast have no
descriptor: they read the plan from device memory, and the GPU part compares the device's FAST cell
table with the cell grid recomputed here.)

GPU part: extraction against the oracle, bit for bit per level, at sizes whose upper levels are single
partial tiles in both directions for k_resize (128 x 32) and k_blur (128 x 128) and whose blurred tile
rows end in a partial 16-byte chunk, in batches of 1, 3 and 5 images (block totals that are no
multiple of 8: the remap's remainder branch).  253 x 199 is the issue's size and the plan accepts it;
its level widths are 253 211 176 146 122 102 85 71 and heights 199 166 138 115 96 80 67 56, so it
holds both kinds of level, multiples of the 16 x 8 tile and not.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from orb_slam2_commit_amd import _lib

LEVELS, RESIZE, BOUNDS, GRIDS, REMAP, XTAB, YTAB = range(1, 8)
LP_OCTREE, LP_CELLS, LP_OCT_LEVELS = 10, 11, 12
RZ_TW, RZ_TH, BLUR_TW, BLUR_TH = 128, 32, 128, 128

GEOMS = [("kitti", 1241, 376, 2000), ("euroc", 752, 480, 1200), ("tum", 640, 480, 1000), ("small", 320, 240, 500)]
PARAMS = (1.2, 8, 20, 7)


def plan(what, w, h, nf, a0=0, a1=0, a2=0):
    L = _lib.lib()
    p = _lib.ExtractorParams(nf, *PARAMS)
    n = L.orbx_debug_launch_plan(C.byref(p), w, h, what, a0, a1, a2, None, 0)
    assert n >= 0, n
    out = np.zeros(n, np.int64)
    assert L.orbx_debug_launch_plan(C.byref(p), w, h, what, a0, a1, a2, _lib.ptr(out), n) == n
    return out


def level_sizes(w, h, sf, nlevels):
    """ORBextractor's float scale table (double product rounded to float per level), its inverse, and
    cvRound((float)cols * mvInvScaleFactor[l]) as in bench.py:level_sizes."""
    scale = [np.float32(1)]
    for _ in range(1, nlevels):
        scale.append(np.float32(np.float64(scale[-1]) * np.float64(np.float32(sf))))
    inv = [np.float32(1) / s for s in scale]
    return [(int(np.rint(np.float32(w) * s)), int(np.rint(np.float32(h) * s))) for s in inv]


def up(v, m):
    return (v + m - 1) // m * m


@pytest.mark.parametrize("name,w,h,nf", GEOMS)
def test_descriptors_match_recomputed_geometry(name, w, h, nf):
    sf, nl, ini, mn = PARAMS
    sizes = level_sizes(w, h, sf, nl)
    lv = plan(LEVELS, w, h, nf).reshape(-1, 8)
    assert [tuple(r[:2]) for r in lv] == sizes
    # pyramid / blurred offsets and the blur tiles, from the sizes alone
    off, boff, tile_begin = [0] * nl, [0] * nl, [0] * nl
    pyr = blur = ntiles = 0
    for l, (lw, lh) in enumerate(sizes):
        off[l] = 0 if l == 0 else pyr
        pyr += lw * lh if l else 0
        boff[l] = blur
        blur += up(up(lw, 16) * up(lh, 8), 256)
        tile_begin[l] = ntiles
        ntiles += -(-lw // BLUR_TW) * -(-lh // BLUR_TH)
    pyr_bytes, blur_bytes = up(pyr, 256), up(blur, 256)
    for l, (lw, lh) in enumerate(sizes):
        assert tuple(lv[l]) == (lw, lh, off[l], boff[l], up(lw, 16), tile_begin[l], -(-lw // BLUR_TW), -(-lh // BLUR_TH))
    # k_resize: sizes, offsets, table offsets; the staging constants from the bound table itself
    rz = plan(RESIZE, w, h, nf).reshape(-1, 16)
    bounds = plan(BOUNDS, w, h, nf).reshape(-1, 2)
    assert len(rz) == nl - 1
    xoff = yoff = boff_i = 0
    spans, rows = [], []
    for i, r in enumerate(rz):
        l = i + 1
        (sw, sh), (dw, dh) = sizes[l - 1], sizes[l]
        ntx, nty = -(-dw // RZ_TW), -(-dh // RZ_TH)
        assert tuple(r[:11]) == (sw, sh, dw, dh, -1 if l == 1 else off[l - 1], off[l], pyr_bytes, xoff, yoff, boff_i,
                                 boff_i + ntx)
        assert tuple(r[14:]) == (ntx, nty)
        bx, by = bounds[boff_i:boff_i + ntx], bounds[boff_i + ntx:boff_i + ntx + nty]
        spans += list(bx[:, 1] - bx[:, 0] + 1)
        rows += list(by[:, 1] - by[:, 0] + 1)
        xoff, yoff, boff_i = xoff + dw, yoff + dh, boff_i + ntx + nty
    assert boff_i == len(bounds)
    stride = max(16, max(up(int(s), 16) for s in spans))
    lc = int(np.ceil(np.log2(stride // 16)))
    assert all(tuple(r[11:14]) == (stride, max(rows), lc) for r in rz)
    assert 16 << lc >= stride and max(rows) <= 64


def fast_cells(sizes):
    """ComputeKeyPointsOctTree's 30-px cell grid (src/ORBextractor.cc:826-880) as the plan lays it out: per
    cell (level, x0, y0, x1, y1, cap, kin) with the detection region inclusive, cap = ceil(w/2) * ceil(h/2)
    candidate slots and kin = min(cap, 4 * ceil(2 * 1.25^level)) of them inline."""
    import math
    f, out = np.float32, []
    for l, (w, h) in enumerate(sizes):
        lo, max_x, max_y = 16, w - 16, h - 16
        width, height = f(max_x - lo), f(max_y - lo)
        ncols, nrows = int(width / f(30)), int(height / f(30))
        if not (width > 0 and height > 0 and ncols > 0 and nrows > 0):
            continue
        wc, hc = math.ceil(width / f(ncols)), math.ceil(height / f(nrows))
        for i in range(nrows):
            ini_y = lo + i * hc
            if ini_y >= max_y - 3:
                continue
            end_y = min(ini_y + hc + 6, max_y)
            for j in range(ncols):
                ini_x = lo + j * wc
                if ini_x >= max_x - 6:
                    continue
                end_x = min(ini_x + wc + 6, max_x)
                x0, y0, x1, y1 = ini_x + 3, ini_y + 3, end_x - 4, end_y - 4
                if x1 < x0 or y1 < y0:
                    continue
                cap = ((x1 - x0 + 2) // 2) * ((y1 - y0 + 2) // 2)
                out.append((l, x0, y0, x1, y1, cap, min(cap, 4 * math.ceil(2 * 1.25 ** l))))
    return out


def octree_smem_bytes(nc, cell_cap, kcap):
    """k_octree's dynamic LDS (orbx_internal.h:octree_smem_bytes), restated."""
    nc, cell_cap, kcap = int(nc), int(cell_cap), int(kcap)
    np2 = 1 << max(nc - 1, 0).bit_length()
    b = 2 * 4 * nc * 2 + 2 * 2 * nc * 4 + nc * 4 * 4 + nc * 4 * 2 + nc * 2 + 2 * nc * 4
    return up(b, 8) + np2 * 8 + (cell_cap + 1) * 4 + 8 * 4 + kcap * 6


@pytest.mark.parametrize("name,w,h,nf", GEOMS + [("odd", 253, 199, 300)])
def test_octree_groups_and_cell_slots(name, w, h, nf):
    """ORBX_LP_OCTREE, ORBX_LP_CELLS, ORBX_LP_OCT_LEVELS: the launch rows hold every level they run within
    tests/cpp/test_plan.cpp:check_octree_groups' LDS bound, and the cells' slots are laid out as the
    recomputed grid says."""
    sf, nl, _, _ = PARAMS
    og = plan(LP_OCTREE, w, h, nf).reshape(-1, 8)
    cells = plan(LP_CELLS, w, h, nf).reshape(-1, 8)
    lv = plan(LP_OCT_LEVELS, w, h, nf).reshape(-1, 8)
    sizes = level_sizes(w, h, sf, nl)
    assert len(lv) == nl
    # cells: the recomputed grid, kin <= cap, logical offsets contiguous
    grid = fast_cells(sizes)
    assert [tuple(c[:5]) + (c[6], c[7]) for c in cells] == grid
    assert (cells[:, 7] <= cells[:, 6]).all() and (cells[:, 7] >= 1).all()
    assert list(cells[:, 5]) == list(np.cumsum([0] + list(cells[:-1, 6])))
    # levels: the border box, and output slots back to back that hold the quota and the first round's children
    oct_off = 0
    for l, (lw, lh) in enumerate(sizes):
        minx, miny, maxx, maxy, n, n_ini, off, cap = (int(v) for v in lv[l])
        assert (minx, miny, maxx, maxy) == (16, 16, lw - 16, lh - 16)
        assert n_ini == max(1, int(np.floor(float(np.float32(maxx - minx) / np.float32(maxy - miny)) + 0.5)))
        assert off == oct_off and cap == max(n + 3, 4 * n_ini)
        oct_off += cap
    assert lv[:, 4].sum() == nf
    # rows: the groups partition the levels, the last row runs them all for batches up to 2 images
    groups, one = og[:-1], og[-1]
    assert 1 <= len(groups) <= 2 and groups[0][0] == 0 and groups[-1][1] == nl
    assert all(groups[i][0] == groups[i - 1][1] for i in range(1, len(groups)))
    assert (one[0], one[1], one[7]) == (0, nl, 2) and (groups[:, 7] == -1).all()
    ncl = [int((cells[:, 0] == l).sum()) for l in range(nl)]
    for l0, l1, nt, node_cap, cell_cap, kcap, smem, _ in og:
        assert nt in (256, 512) and node_cap % 64 == 0 and node_cap <= 8192 and kcap >= 64 and kcap % 64 == 0
        assert smem == octree_smem_bytes(node_cap, cell_cap, kcap) <= 160 * 1024 - 1024
        for l in range(l0, l1):
            assert node_cap >= lv[l][7] and cell_cap >= ncl[l]


@pytest.mark.parametrize("name,w,h,nf", GEOMS + [("odd", 253, 199, 300)])
def test_bound_tables_match_coefficient_tables(name, w, h, nf):
    rz = plan(RESIZE, w, h, nf).reshape(-1, 16)
    bounds = plan(BOUNDS, w, h, nf).reshape(-1, 2)
    for i, r in enumerate(rz):
        l, dw, dh, bx_off, by_off, ntx, nty = i + 1, r[2], r[3], r[9], r[10], r[14], r[15]
        X, Y = plan(XTAB, w, h, nf, l).reshape(-1, 4), plan(YTAB, w, h, nf, l).reshape(-1, 4)
        assert len(X) == dw and len(Y) == dh
        for c in range(ntx):
            assert tuple(bounds[bx_off + c]) == (X[c * RZ_TW][0], X[min((c + 1) * RZ_TW, dw) - 1][1])
        for c in range(nty):
            assert tuple(bounds[by_off + c]) == (Y[c * RZ_TH][0], Y[min((c + 1) * RZ_TH, dh) - 1][1])
        # every footprint lies inside the source level
        assert bounds[bx_off:bx_off + ntx].min() >= 0 and bounds[bx_off:bx_off + ntx, 1].max() < r[0]
        assert bounds[by_off:by_off + nty].min() >= 0 and bounds[by_off:by_off + nty, 1].max() < r[1]


def _real_grids():
    """The k_resize and k_blur grids of the plans (orbx_debug_launch_plan), and the k_fast grids from the
    recomputed cell grid (two cells per wave, one launch for all cells and one per half as stand-ins for
    the launch groups)."""
    grids = []
    for _, w, h, nf in GEOMS + [("odd", 253, 199, 300)]:
        ncells = len(fast_cells(level_sizes(w, h, PARAMS[0], PARAMS[1])))
        for n in (1, 3, 5, 512):
            grids += [tuple(int(v) for v in g) for g in plan(GRIDS, w, h, nf, n).reshape(-1, 3)]
            grids += [((ncells + 1) // 2, n, 1), ((ncells // 2 + 1) // 2, n, 1)]
    return grids


def test_remap_constants_exhaustive():
    grids = sorted(set(_real_grids() + [(gx, gy, gz) for gx in (1, 7, 10, 97) for gy in (1, 3, 12)
                                        for gz in (1, 3, 5, 512)]))
    for gx, gy, gz in grids:
        rgx, rgy, q, r, mx, sx, my, sy = (int(v) for v in plan(REMAP, 1, 1, 0, gx, gy, gz))
        total = gx * gy * gz
        assert (rgx, rgy, q, r) == (gx, gy, total >> 3, total & 7)
        assert 0 < mx < 1 << 32 and 0 < my < 1 << 32 and sx < 32 and sy < 32
        l = np.arange(total, dtype=np.uint64)

        def div(v, m, s):  # the kernels' 32-bit form: mulhi(2v + 1, m) >> s
            n = 2 * v + 1
            assert int(n.max()) < 1 << 32
            return ((n * np.uint64(m)) >> np.uint64(32)) >> np.uint64(s)

        qx = div(l, mx, sx)
        z = div(qx, my, sy)
        assert np.array_equal(qx, l // np.uint64(gx)), (gx, gy, gz)
        assert np.array_equal(l - qx * np.uint64(gx), l % np.uint64(gx))
        assert np.array_equal(qx - z * np.uint64(gy), (l // np.uint64(gx)) % np.uint64(gy)), (gx, gy, gz)
        assert np.array_equal(z, l // np.uint64(gx * gy)), (gx, gy, gz)
        # the hardware-id -> logical-id step stays the bijection of xcd_block()
        hw = np.arange(total, dtype=np.int64)
        x = hw & 7
        assert np.array_equal(np.sort(x * q + np.minimum(x, r) + (hw >> 3)), hw)


def test_launch_plan_argument_checks():
    L = _lib.lib()
    p = _lib.ExtractorParams(500, *PARAMS)
    assert L.orbx_debug_launch_plan(None, 320, 240, LEVELS, 0, 0, 0, None, 0) == -1
    assert L.orbx_debug_launch_plan(C.byref(p), 320, 240, 99, 0, 0, 0, None, 0) == -1
    assert L.orbx_debug_launch_plan(C.byref(p), 320, 240, XTAB, 0, 0, 0, None, 0) == -1  # level 0 has no table
    assert L.orbx_debug_launch_plan(C.byref(p), 320, 240, REMAP, 0, 1, 1, None, 0) == -1
    assert L.orbx_debug_launch_plan(C.byref(p), 320, 240, REMAP, 1 << 12, 1 << 12, 1 << 12, None, 0) == -1  # > 2^30 blocks
    assert L.orbx_debug_launch_plan(C.byref(p), 5000, 240, LEVELS, 0, 0, 0, None, 0) == -5


# ------------------------------------------------------------------------------------------- GPU
DBG_BLUR, DBG_CELL_COUNTS, DBG_CELL_TABLE, DBG_CAND = 1, 2, 3, 4
SIZES = {"small": (320, 240, 500), "odd": (253, 199, 300)}


def _dbg(ex, what, image=0, arg=0, dtype=np.int32):
    L = _lib.lib()
    n = L.orbx_debug_copy(ex._h, what, image, arg, None, 0)
    assert n >= 0, n
    buf = np.zeros(max(n, 1), np.uint8)
    L.orbx_debug_copy(ex._h, what, image, arg, _lib.ptr(buf), n)
    return buf[:n].view(dtype)


@functools.lru_cache(maxsize=None)
def _reference(size, seed, stress):
    """Image `seed` of a size and everything the oracle says about it, computed once."""
    import oracle
    from orb_slam2_commit_amd import synth
    w, h, nf = SIZES[size]
    img = synth.stereo_pair(seed, w, h, stress=stress)[0]
    ref = oracle.extract(oracle.params(nf, *PARAMS), img)
    levels = [ref.level(l) for l in range(PARAMS[1])]
    blurred = [oracle.gaussian_blur7(lv) for lv in levels]
    return img, ref, levels, blurred


def _check_batch(gpu, size, n, stress):
    import oracle
    import torch
    from orb_slam2_commit_amd import ORBextractor
    w, h, nf = SIZES[size]
    refs = [_reference(size, 60 + i, stress) for i in range(n)]
    ex = ORBextractor(nf, *PARAMS)
    cap = ex.max_keypoints(w, h)
    d_img = torch.from_numpy(np.stack([r[0] for r in refs])).to(gpu)
    kps = torch.zeros((n, cap, 28), dtype=torch.uint8, device=gpu)
    desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device=gpu)
    cnt = torch.zeros(n, dtype=torch.int32, device=gpu)
    ex.extract_batch_device(d_img, kps, desc, cnt, torch.cuda.current_stream())
    torch.cuda.synchronize()
    cnt, kps, desc = cnt.cpu().numpy(), kps.cpu().numpy(), desc.cpu().numpy()
    cells = _dbg(ex, DBG_CELL_TABLE).reshape(-1, 8)
    grid = fast_cells(level_sizes(w, h, PARAMS[0], PARAMS[1]))
    assert len(cells) == len(grid) > 0
    # the device plan's cell table is the recomputed grid; its candidate slots are the caps back to back
    assert [tuple(c[:5]) + (c[6],) for c in cells] == [g[:6] for g in grid]
    assert list(cells[:, 5]) == list(np.cumsum([0] + [g[5] for g in grid[:-1]]))
    kin = [g[6] for g in grid]
    n_min_all = n_over_all = 0
    for i, (img, ref, levels, blurred) in enumerate(refs):
        for l in range(PARAMS[1]):
            assert np.array_equal(ex.pyramid_level(l, i), levels[l]), (i, l, "pyramid")
            got = _dbg(ex, DBG_BLUR, i, l, np.uint8).reshape(levels[l].shape)
            assert np.array_equal(got, blurred[l]), (i, l, "blurred")
        counts = _dbg(ex, DBG_CELL_COUNTS, i)
        cand = _dbg(ex, DBG_CAND, i, dtype=np.uint32)
        for ci, (lvl, x0, y0, x1, y1, off, ccap, _) in enumerate(cells):
            win = levels[lvl][y0 - 3:y1 + 4, x0 - 3:x1 + 4]
            exp = oracle.fast_window(win, PARAMS[2])
            if len(exp) == 0:
                exp = oracle.fast_window(win, PARAMS[3])
                n_min_all += 1
            n_over_all += len(exp) > kin[ci]
            packed = (exp[:, 2].astype(np.uint32) << 24) | ((exp[:, 1] + y0 - 3).astype(np.uint32) << 12) | \
                (exp[:, 0] + x0 - 3).astype(np.uint32)
            assert np.array_equal(cand[off:off + counts[ci]], packed), (i, ci, "FAST candidates")
        assert cnt[i] == len(ref.keypoints), i
        assert kps[i, :cnt[i]].tobytes() == ref.keypoints.tobytes(), (i, "keypoints")
        assert np.array_equal(desc[i, :cnt[i]], ref.descriptors), (i, "descriptors")
    return n_min_all, n_over_all, n * len(cells)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("size", ["small", "odd"])
def test_batch_extraction_bitexact_per_level(gpu, size, n):
    """Scene images: in every batch some cells find nothing at iniThFAST and run the minThFAST pass, and
    some keep more survivors than their inline slots hold (both counted from the oracle's windows)."""
    n_min, n_over, _ = _check_batch(gpu, size, n, False)
    assert n_min > 0 and n_over > 0, (n_min, n_over)


@pytest.mark.gpu
def test_batch_extraction_stress_images(gpu):
    """Uniform-noise images: dense FAST responses, every cell past its inline candidate slots (none takes
    the minThFAST pass on noise: the scene images above cover that)."""
    n_min, n_over, n_cells = _check_batch(gpu, "odd", 3, True)
    assert n_over > n_cells // 2, (n_over, n_cells)


@pytest.mark.gpu
def test_stereo_frames_small(gpu):
    import oracle
    import torch
    from orb_slam2_commit_amd import ORBextractor, synth
    bf, fx = 386.1448, 718.856
    n, (w, h, nf) = 3, SIZES["small"]
    pairs = [synth.stereo_pair(70 + i, w, h) for i in range(n)]
    ex = ORBextractor(nf, *PARAMS)
    cap = ex.max_keypoints(w, h)
    d = torch.from_numpy(np.stack([im for pr in pairs for im in pr])).to(gpu)
    kps = torch.zeros((2 * n, cap, 28), dtype=torch.uint8, device=gpu)
    desc = torch.zeros((2 * n, cap, 32), dtype=torch.uint8, device=gpu)
    cnt = torch.zeros(2 * n, dtype=torch.int32, device=gpu)
    uR = torch.zeros((n, cap), dtype=torch.float32, device=gpu)
    dep = torch.zeros((n, cap), dtype=torch.float32, device=gpu)
    nm = torch.zeros(n, dtype=torch.int32, device=gpu)
    ex.stereo_frames_device(d, kps, desc, cnt, bf, bf / fx, uR, dep, nm, torch.cuda.current_stream())
    torch.cuda.synchronize()
    p = oracle.params(nf, *PARAMS)
    for f in range(n):
        oL, oR = oracle.extract(p, pairs[f][0]), oracle.extract(p, pairs[f][1])
        ouR, odep = oracle.stereo_match(p, oL, oR, bf, bf / fx)
        nL = int(cnt[2 * f])
        assert nL == len(oL.keypoints) and int(cnt[2 * f + 1]) == len(oR.keypoints)
        assert kps[2 * f, :nL].cpu().numpy().tobytes() == oL.keypoints.tobytes()
        assert np.array_equal(uR[f, :nL].cpu().numpy().view(np.uint32), ouR.view(np.uint32))
        assert np.array_equal(dep[f, :nL].cpu().numpy().view(np.uint32), odep.view(np.uint32))
        assert int(nm[f]) == int((ouR >= 0).sum())

"""k_fast per launch group: every instantiated (S, RP, NK) kernel, cell by cell against the oracle.

k_fast<S, RP, NK> stages a cell's window with NK 16-B loads per lane (21 window rows per load at
S = 40 / 48), NK chosen per launch group from its tallest window, and walks the region 8 rows per
compass trip with the last, partial trip peeled.  One-level extractors on small images put every cell
at a chosen width W and height H (the level's border region is a whole number of cells), so each
case lands in a known kernel: window heights H + 6 on both sides of the load-count boundaries
(42 / 43 rows at S = 40 and 48, 48 / 49 at S = 80), H = 31 .. 40, and H % 8 in {0, 1, 2, 7} for the
peeled trip.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from orb_slam2_commit_amd import ORBextractor, synth
from orb_slam2_commit_amd import _lib

pytestmark = pytest.mark.gpu

DBG_CELL_COUNTS, DBG_CELL_TABLE, DBG_CAND = 2, 3, 4
LP_FAST = 9
PARAMS = (200, 1.2, 1, 20, 7)  # one level: the image is the level
BORDER = 32  # the level's FAST region is (w - 32) x (h - 32)

# (cell width W, cell height H, cell columns, cell rows) -> the kernel k_fast<S, RP, NK> it must run.
# W x H is the first cell; the last column / row of a level is 6 narrower / shorter (its window is
# clipped to the region), so H - 6 occurs as well.
CASES = [
    ((31, 31, 2, 2), (40, 2, 2)),
    ((33, 32, 2, 2), (40, 1, 2)),
    ((35, 33, 2, 2), (48, 1, 2)),
    ((32, 34, 2, 2), (40, 2, 2)),
    ((34, 35, 2, 2), (40, 1, 2)),
    ((32, 36, 2, 2), (40, 2, 2)),  # 42 window rows: two loads
    ((32, 37, 2, 2), (40, 2, 3)),  # 43: three
    ((34, 36, 2, 2), (40, 1, 2)),
    ((34, 37, 2, 2), (40, 1, 3)),
    ((42, 36, 2, 2), (48, 1, 2)),
    ((42, 37, 2, 2), (48, 1, 3)),
    ((33, 38, 2, 2), (40, 1, 3)),
    ((35, 39, 2, 2), (48, 1, 3)),
    ((31, 40, 2, 2), (40, 2, 3)),
    ((44, 42, 2, 2), (80, 1, 4)),  # 48 window rows at 12 per load: four loads
    ((44, 43, 2, 2), (80, 1, 5)),  # 49: five
]
# every k_fast the library instantiates (no cell grid makes a window taller than 59 rows: 3 loads at
# S = 40 / 48, 5 at S = 80)
KERNELS = {(40, 2, 2), (40, 2, 3), (40, 1, 2), (40, 1, 3), (48, 1, 2), (48, 1, 3), (80, 1, 4), (80, 1, 5)}
BOUNDARY = {40: {(42, 2), (43, 3)}, 48: {(42, 2), (43, 3)}, 80: {(48, 4), (49, 5)}}


def _size(case):
    W, H, nx, ny = case
    return BORDER + W * nx, BORDER + H * ny


def _dbg(ex, what, dtype=np.int32):
    L = _lib.lib()
    n = L.orbx_debug_copy(ex._h, what, 0, 0, None, 0)
    assert n >= 0, n
    buf = np.zeros(n, np.uint8)
    L.orbx_debug_copy(ex._h, what, 0, 0, _lib.ptr(buf), n)
    return buf.view(dtype)


def _fast_groups(w, h):
    L = _lib.lib()
    nf, sf, nl, ini, mn = PARAMS
    p = _lib.ExtractorParams(nf, sf, nl, ini, mn)
    n = L.orbx_debug_launch_plan(C.byref(p), w, h, LP_FAST, 0, 0, 0, None, 0)
    assert n > 0 and n % 8 == 0, n
    out = np.zeros(n, np.int64)
    assert L.orbx_debug_launch_plan(C.byref(p), w, h, LP_FAST, 0, 0, 0, _lib.ptr(out), n) == n
    return out.reshape(-1, 8)


def test_cases_cover_kernels():
    kernels, heights = set(), set()
    for case, kern in CASES:
        w, h = _size(case)
        g = _fast_groups(w, h)
        assert len(g) == 1 and g[0][0] == 0 and g[0][1] == case[2] * case[3], g  # one group, every cell
        assert tuple(int(v) for v in g[0][2:5]) == kern, (case, g[0][2:5])
        kernels.add(kern)
        heights.add(case[1])
    assert kernels == KERNELS
    assert set(range(31, 41)) <= heights
    assert {0, 1, 2, 7} <= {H % 8 for H in heights}
    # both sides of the load-count boundary of every stride
    for s, want in BOUNDARY.items():
        rows = {(c[1] + 6, k[2]) for c, k in CASES if k[0] == s}
        assert want <= rows, (s, sorted(rows))


@pytest.fixture(scope="module")
def runs(gpu):
    """Per case: the oracle's extraction and the library's cell table, counts and candidates."""
    p = oracle.params(*PARAMS)
    out = []
    for (W, H, nx, ny), _ in CASES:
        w, h = _size((W, H, nx, ny))
        ex = ORBextractor(*PARAMS)
        both = []
        # a smooth scene (few corners: most cells fall back to minThFAST) and a noisy one (hundreds)
        for stress in (False, True):
            img = synth.stereo_pair(60 + W + H, w, h, stress=stress)[0]
            ex(img)
            both.append((oracle.extract(p, img), _dbg(ex, DBG_CELL_TABLE).reshape(-1, 8).copy(),
                         _dbg(ex, DBG_CELL_COUNTS).copy(), _dbg(ex, DBG_CAND, np.uint32).copy()))
        out.append(both)
    return out


def test_cell_tables_cover_heights(runs):
    heights = set()
    for (case, _), both in zip(CASES, runs):
        W, H, nx, ny = case
        cells = both[0][1]
        assert np.array_equal(cells, both[1][1])
        # the geometry is the one the case names: nx x ny cells, the first (and largest) W x H
        assert len(cells) == nx * ny
        ws, hs = cells[:, 3] - cells[:, 1] + 1, cells[:, 4] - cells[:, 2] + 1
        assert ws[0] == W and hs[0] == H and ws.max() == W and hs.max() == H, cells[:, 1:5]
        assert ws.max() > 32 or case[0] <= 32
        heights |= set(int(v) for v in hs)
    assert set(range(31, 41)) <= heights, sorted(heights)
    assert {0, 1, 2, 7} <= {H % 8 for H in heights}


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["%dx%d" % c[0][:2] for c in CASES])
def test_fast_cells_per_kernel(runs, idx):
    for ref, cells, counts, cand in runs[idx]:
        bad, total = 0, 0
        for ci, (lvl, x0, y0, x1, y1, off, cap, _) in enumerate(cells):
            im = ref.level(lvl)
            win = im[y0 - 3:y1 + 4, x0 - 3:x1 + 4]  # the reference's FAST window [iniY,maxY) x [iniX,maxX)
            got = cand[off:off + counts[ci]]
            exp = oracle.fast_window(win, PARAMS[3])
            if len(exp) == 0:
                exp = oracle.fast_window(win, PARAMS[4])
            exp_packed = (exp[:, 2].astype(np.uint32) << 24) | ((exp[:, 1] + y0 - 3).astype(np.uint32) << 12) | \
                (exp[:, 0] + x0 - 3).astype(np.uint32)
            total += len(exp_packed)
            if not np.array_equal(got, exp_packed):
                bad += 1
        assert total > 0, "no corner in any cell: the case checks nothing"
        assert bad == 0, "%d/%d cells differ" % (bad, len(cells))

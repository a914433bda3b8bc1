"""k_fast's packed compass trip: two sub-steps per register, cell by cell against the oracle.

The compass test holds sub-steps u and u + 1 of an 8-row trip in the two 16-bit halves of each
register (rows y and y + 2 of a column where a compass instruction covers two rows of up to 32 columns,
RP = 2; rows y and y + 1 where it covers one row, RP = 1), so what can go wrong sits at the pairing:
the peeled last trip with an odd number of sub-steps, the last sub-step with only its first row inside
the region, lanes past the cell's width, and differences that use the whole signed 16-bit range of the
packed arithmetic.  One-level extractors on small images put every cell at a chosen W x H, as
test_gpu_fast_groups.py does (the last column / row of cells is 6 narrower / shorter):

* H = 31 .. 38 at W = 31 (RP = 2) and W = 34 (RP = 1): with the 6-shorter last row every residue
  H % 8 occurs in both, i.e. for RP = 2 one unpaired sub-step ({1, 2}), one pair ({3, 4}), a pair plus
  one ({5, 6}) and two pairs ({7, 0}), each with and without a half-filled last sub-step;
* W = 32 (every lane of a half-wave carries a pixel), W = 31 and the narrower last column (idle lanes
  must not hit), W = 33 (the first RP = 1 width);
* per case two synthetic scenes and a crafted image: 255-squares on 0 and 0-squares on 255 (differences
  of +-255), ring patterns at exactly c +- th and c +- (th + 1) for th = 20 and th = 7, and a cell of
  faint noise that holds no corner at either threshold;
* one extractor at iniThFAST = 200, minThFAST = 1 on the crafted image: the fallback pass at a tiny
  threshold puts almost every pixel of the noise cell on the compass list.
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
PARAMS = (200, 1.2, 1, 20, 7)      # one level: the image is the level
PARAMS_LOW = (200, 1.2, 1, 200, 1)  # nearly every cell falls back to threshold 1
BORDER = 32  # the level's FAST region is (w - 32) x (h - 32) and starts at (19, 19)
ORIGIN = 19

# (cell width W, cell height H); 2 x 2 cells each
CASES = [(31, H) for H in range(31, 39)] + [(34, H) for H in range(31, 39)] + \
        [(32, 32), (32, 35), (33, 33), (33, 36)]
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def _size(case):
    return BORDER + 2 * case[0], BORDER + 2 * case[1]


def _dbg(ex, what, dtype=np.int32):
    L = _lib.lib()
    n = L.orbx_debug_copy(ex._h, what, 0, 0, None, 0)
    assert n >= 0, n
    buf = np.zeros(n, np.uint8)
    L.orbx_debug_copy(ex._h, what, 0, 0, _lib.ptr(buf), n)
    return buf.view(dtype)


def _fast_groups(w, h):
    L = _lib.lib()
    p = _lib.ExtractorParams(*PARAMS)
    n = L.orbx_debug_launch_plan(C.byref(p), w, h, LP_FAST, 0, 0, 0, None, 0)
    assert n > 0 and n % 8 == 0, n
    out = np.zeros(n, np.int64)
    assert L.orbx_debug_launch_plan(C.byref(p), w, h, LP_FAST, 0, 0, 0, _lib.ptr(out), n) == n
    return out.reshape(-1, 8)


def crafted(W, H):
    """The crafted image of a 2 x 2 grid of W x H cells (cell regions start at (19, 19)).

    Top-left cell: 6 x 6 squares and single pixels of 255 on 0 in its left half, of 0 on 255 in its
    right half.
    Bottom-left cell: on a flat 100, four centres whose whole ring is at 100 + d for d = 20, 21, -20, -21
    (a corner at threshold 20 iff |d| = 21).  Top-right cell: the same for d = 7, 8, -7, -8, so the cell
    holds no corner at 20 and the ones with |d| = 8 at 7.  Bottom-right cell: noise in 100 .. 103, no
    corner at 7 or 20 and compass hits nearly everywhere at 1."""
    w, h = BORDER + 2 * W, BORDER + 2 * H
    xs, ys = ORIGIN + W, ORIGIN + H  # first column / row of the second cells
    img = np.full((h, w), 100, np.uint8)
    # top-left
    xm = ORIGIN + W // 2
    img[:ys - 4, :xm] = 0
    img[:ys - 4, xm:xs - 4] = 255
    for y in range(ORIGIN + 2, ys - 4 - 8, 12):
        for x in range(ORIGIN + 2, xs - 4 - 8, 12):
            if x + 6 <= xm or x >= xm:
                img[y:y + 6, x:x + 6] = 255 if x < xm else 0
            # a square's corner pixels tie with their neighbours at score 254 and strict NMS drops them
            # all; a single pixel in the gap is a corner whose neighbours are none
            if x + 10 <= xm or (x >= xm and x + 10 <= xs - 4):
                img[y + 9, x + 9] = 255 if x < xm else 0
    # ring patterns: 2 x 2 centres, 10 apart, 6 inside the cell
    def rings(x0, y0, ds):
        for k, d in enumerate(ds):
            cx, cy = x0 + 6 + 10 * (k & 1), y0 + 6 + 10 * (k >> 1)
            for dx, dy in RING:
                img[cy + dy, cx + dx] = 100 + d
    rings(ORIGIN, ys, (20, 21, -20, -21))
    rings(xs, ORIGIN, (7, 8, -7, -8))
    # bottom-right
    rng = np.random.default_rng(W * 64 + H)
    img[ys - 4:, xs - 4:] = 100 + rng.integers(0, 4, (h - ys + 4, w - xs + 4), dtype=np.uint8)
    return img


def _cells_vs_oracle(ref, cells, counts, cand, ini, mn):
    """(cells that differ, cells with a corner, cells without) against oracle.fast_window."""
    bad, some, none = 0, 0, 0
    for ci, (lvl, x0, y0, x1, y1, off, cap, _) in enumerate(cells):
        im = ref.level(lvl)
        win = im[y0 - 3:y1 + 4, x0 - 3:x1 + 4]  # the reference's FAST window [iniY,maxY) x [iniX,maxX)
        got = cand[off:off + counts[ci]]
        exp = oracle.fast_window(win, ini)
        if len(exp) == 0:
            exp = oracle.fast_window(win, mn)
        exp_packed = (exp[:, 2].astype(np.uint32) << 24) | ((exp[:, 1] + y0 - 3).astype(np.uint32) << 12) | \
            (exp[:, 0] + x0 - 3).astype(np.uint32)
        assert len(exp_packed) <= cap  # the comparison below is of whole lists
        some += len(exp_packed) > 0
        none += len(exp_packed) == 0
        bad += not np.array_equal(got, exp_packed)
    return bad, some, none


def _run(ex, p, img):
    ex(img)
    return (oracle.extract(p, img), _dbg(ex, DBG_CELL_TABLE).reshape(-1, 8).copy(),
            _dbg(ex, DBG_CELL_COUNTS).copy(), _dbg(ex, DBG_CAND, np.uint32).copy())


@pytest.fixture(scope="module")
def runs(gpu):
    """Per case: (the synthetic scenes and the crafted image at 20 / 7, the crafted image at 200 / 1)."""
    p, plow = oracle.params(*PARAMS), oracle.params(*PARAMS_LOW)
    out = []
    for W, H in CASES:
        w, h = _size((W, H))
        ex, exlow = ORBextractor(*PARAMS), ORBextractor(*PARAMS_LOW)
        imgs = [synth.stereo_pair(90 + W + H, w, h, stress=False)[0],
                synth.stereo_pair(90 + W + H, w, h, stress=True)[0], crafted(W, H)]
        out.append(([_run(ex, p, im) for im in imgs], _run(exlow, plow, imgs[2])))
    return out


def test_cases_cover_pairings(gpu):
    """The launch plan runs the RP the case is meant for."""
    for W, H in CASES:
        g = _fast_groups(*_size((W, H)))
        assert len(g) == 1 and g[0][0] == 0 and g[0][1] == 4, g
        assert int(g[0][3]) == (2 if W <= 32 else 1), (W, H, g[0][2:5])
    assert {W for W, _ in CASES} >= {31, 32, 33, 34}


def test_cell_tables_cover_residues(runs):
    res = {1: set(), 2: set()}
    widths = set()
    for (W, H), (both, _) in zip(CASES, runs):
        cells = both[0][1]
        assert len(cells) == 4
        ws, hs = cells[:, 3] - cells[:, 1] + 1, cells[:, 4] - cells[:, 2] + 1
        assert cells[0, 1] == ORIGIN and cells[0, 2] == ORIGIN
        assert ws[0] == W and hs[0] == H and ws.max() == W and hs.max() == H, cells[:, 1:5]
        assert ws.min() == W - 6 and hs.min() == H - 6, cells[:, 1:5]
        res[2 if W <= 32 else 1] |= {int(v) % 8 for v in hs}
        widths |= {int(v) for v in ws}
    # RP = 2: one unpaired sub-step, one pair, a pair plus one, two pairs, each with the last sub-step
    # whole and half inside; RP = 1: every count of rows in the peeled trip
    assert res[2] == set(range(8)) and res[1] == set(range(8)), res
    assert {25, 26, 27, 31, 32, 33} <= widths, sorted(widths)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["%dx%d" % c for c in CASES])
def test_packed_cells(runs, idx):
    both, _ = runs[idx]
    for k, (ref, cells, counts, cand) in enumerate(both):
        bad, some, none = _cells_vs_oracle(ref, cells, counts, cand, PARAMS[3], PARAMS[4])
        assert some > 0, "no corner in any cell: the case checks nothing"
        if k == 2:  # the crafted image: the square cell and both ring cells have corners, the noise cell none
            assert some == 3 and none == 1, (some, none)
        assert bad == 0, "image %d: %d/%d cells differ" % (k, bad, len(cells))


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["%dx%d" % c for c in CASES])
def test_packed_cells_tiny_threshold(runs, idx):
    ref, cells, counts, cand = runs[idx][1]
    bad, some, _ = _cells_vs_oracle(ref, cells, counts, cand, PARAMS_LOW[3], PARAMS_LOW[4])
    # the squares reach 200; the noise cell only has corners in the fallback pass at 1
    assert some >= 2, some
    assert bad == 0, "%d/%d cells differ" % (bad, len(cells))


def test_crafted_image_reaches_the_extremes():
    """The crafted image holds what its docstring says (checked on the oracle alone)."""
    W, H = 31, 33
    img = crafted(W, H).astype(np.int32)
    xs, ys = ORIGIN + W, ORIGIN + H
    # a 0 / 255 edge between horizontally adjacent pixels, both ways
    dx = img[ORIGIN:ys - 4, 1:xs - 4] - img[ORIGIN:ys - 4, :xs - 5]
    assert dx.max() == 255 and dx.min() == -255
    for x0, y0, ds, th in ((ORIGIN, ys, (20, 21, -20, -21), 20), (xs, ORIGIN, (7, 8, -7, -8), 7)):
        win = img[y0 - 3:y0 + 25 + 3, x0 - 3:x0 + 25 + 3].astype(np.uint8)
        got = {(int(x), int(y)) for x, y, _ in oracle.fast_window(win, th)}
        for k, d in enumerate(ds):
            c = (3 + 6 + 10 * (k & 1), 3 + 6 + 10 * (k >> 1))
            assert img[y0 + c[1] - 3, x0 + c[0] - 3] == 100
            assert {int(img[y0 + c[1] - 3 + dy, x0 + c[0] - 3 + dx_]) for dx_, dy in RING} == {100 + d}
            if abs(d) == th:
                assert c not in got, (d, th)
    noise = img[ys:, xs:].astype(np.uint8)
    assert len(oracle.fast_window(noise, 7)) == 0 and len(oracle.fast_window(noise, 1)) > 0

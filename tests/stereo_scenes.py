"""Crafted stereo scenes: small image pairs plus INJECTED keypoints and descriptors that put a left
keypoint on every exit and boundary of Frame::ComputeStereoMatches (tests/test_stereo_literal.py).

Every pyramid is an ordinary extraction of the scene's image (level 0 is the image itself, so octave-0
keypoints see exactly the pixels written here).  A scene is a dict: name, params (nfeatures, scale,
nlevels), L, R (uint8 images), kL, dL, kR, dR, bf, baseline, and `claims`: left index -> the exit codes
(stereo_literal.EXITS) the scene is built to reach there; `uR_near`: left index -> the uRight a correct
winner gives (within one pixel).  The CPU tests check every claim with the literal before the GPU tests
use the scenes.
"""
import functools

import numpy as np

import oracle
import stereo_literal as lit

F32 = np.float32
KP = oracle.KEYPOINT_DTYPE
W, H = 320, 240
BF, BASELINE = 40.0, 0.5  # maxD = 80
PARAM_SETS = ((1.2, 8), (1.5, 4), (1.1, 12), (1.2, 1))
PAST_ORB = ("endu", "guard", "edgeinc", "neg", "far", "clamp", "ok")  # the Hamming stage found a match
ACCEPT = ("clamp", "ok")


# ------------------------------------------------------------------ helpers
def texture(seed, w=W, h=H):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def shifted(L, d, seed, noise=6):
    """right(x) = left(x + d) (a point at uL appears at uL - d), plus uniform noise of +-noise."""
    g = np.random.default_rng(seed)
    R = np.roll(L, -d, axis=1).astype(np.int16) + g.integers(-noise, noise + 1, L.shape)
    return np.clip(R, 0, 255).astype(np.uint8)


def rand_desc(g):
    return g.integers(0, 256, 32, dtype=np.uint8)


def flip_bits(d, bits):
    """d with the listed bit positions (0..255) flipped: Hamming distance len(bits) from d."""
    out = d.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def next_up(x):
    return F32(np.nextafter(F32(x), F32(np.inf)))


def next_down(x):
    return F32(np.nextafter(F32(x), F32(-np.inf)))


def first_x_rounding_to(target, level, scale, nlevels):
    """The smallest float32 x with round(x * inv_scale[level]) >= target (the float just below rounds to
    target - 1): where the rounding of x * inv_scale decides a border test at a level > 0."""
    sc, inv = lit.scale_factors(scale, nlevels)
    x = F32((target - 0.5) * float(sc[level]))
    while lit.c_round(x * inv[level]) >= target:
        x = next_down(x)
    while lit.c_round(x * inv[level]) < target:
        x = next_up(x)
    return x


class Builder:
    def __init__(self, name, L, R, scale=1.2, nlevels=8, bf=BF, baseline=BASELINE, nfeatures=200):
        self.name, self.L, self.R = name, np.ascontiguousarray(L), np.ascontiguousarray(R)
        self.params = (nfeatures, scale, nlevels)
        self.bf, self.baseline = bf, baseline
        self.left_kps, self.left_desc, self.right_kps, self.right_desc = [], [], [], []
        self.claims, self.uR_near = {}, {}

    def left(self, x, y, octave, desc, claim=None, uR_near=None):
        self.left_kps.append((F32(x), F32(y), int(octave)))
        self.left_desc.append(np.asarray(desc, np.uint8))
        i = len(self.left_kps) - 1
        if claim is not None:
            self.claims[i] = (claim,) if isinstance(claim, str) else tuple(claim)
        if uR_near is not None:
            self.uR_near[i] = float(uR_near)
        return i

    def right(self, x, y, octave, desc):
        self.right_kps.append((F32(x), F32(y), int(octave)))
        self.right_desc.append(np.asarray(desc, np.uint8))
        return len(self.right_kps) - 1

    def pair(self, g, uL, vL, uR, octave=0, claim=None, uR_near=None, vR=None):
        d = rand_desc(g)
        self.right(uR, vL if vR is None else vR, octave, d)
        return self.left(uL, vL, octave, d, claim, uR_near)

    @staticmethod
    def _records(kps):
        a = np.zeros(len(kps), KP)
        for i, (x, y, o) in enumerate(kps):
            a[i]["x"], a[i]["y"], a[i]["octave"] = x, y, o
            a[i]["size"], a[i]["angle"], a[i]["response"], a[i]["class_id"] = 31.0, 0.0, 1.0, -1
        return a

    def scene(self):
        h, w = self.L.shape
        for x, y, o in self.left_kps + self.right_kps:  # what orbx_debug_stereo_keypoints accepts
            assert 0 <= x < w and 0 <= y < h and 0 <= o < self.params[2], (self.name, x, y, o)
        return {"name": self.name, "params": self.params, "L": self.L, "R": self.R,
                "kL": self._records(self.left_kps), "dL": np.array(self.left_desc, np.uint8).reshape(-1, 32),
                "kR": self._records(self.right_kps), "dR": np.array(self.right_desc, np.uint8).reshape(-1, 32),
                "bf": self.bf, "baseline": self.baseline, "claims": dict(self.claims),
                "uR_near": dict(self.uR_near)}


def background(b, g, n, d, rows, n_heavy=0, heavy_rows=None):
    """n octave-0 pairs on a pair of images shifted by d: the right keypoint a few pixels off the true
    match, which the SAD search recovers (accepted matches with SAD > 0, a positive median).  n_heavy more
    in `heavy_rows`, where the right image carries heavy noise: accepted, then removed by the median
    filter."""
    w = b.L.shape[1]
    for _ in range(n):
        uL = float(g.integers(110, w - 30)) + float(g.integers(0, 4)) * 0.25
        vL = float(g.integers(rows[0], rows[1])) + float(g.integers(0, 4)) * 0.25
        b.pair(g, uL, vL, uL - d + int(g.integers(-3, 4)), 0)
    for _ in range(n_heavy):
        uL = float(g.integers(110, w - 30))
        vL = float(g.integers(heavy_rows[0] + 6, heavy_rows[1] - 6))
        b.pair(g, uL, vL, uL - d + int(g.integers(-2, 3)), 0)


def heavy_noise(R, rows, seed, amp=70):
    g = np.random.default_rng(seed)
    R = R.astype(np.int16)
    R[rows[0]:rows[1]] += g.integers(-amp, amp + 1, R[rows[0]:rows[1]].shape)
    return np.clip(R, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ the scenes
def scene_background(seed, scale=1.2, nlevels=8, n=40, n_heavy=5, name=None):
    """Accepted matches (ok), some of which the median filter removes (median)."""
    g = np.random.default_rng(seed)
    L = texture(seed)
    R = heavy_noise(shifted(L, 7, seed + 1), (200, 240), seed + 2)
    b = Builder(name or "background_s%g_n%d_%d" % (scale, nlevels, n), L, R, scale, nlevels)
    background(b, g, n, 7, (12, 190), n_heavy, (200, 240))
    return b.scene()


def scene_clamp(seed):
    """Rows 0..119 are mirror-symmetric about column c in both images, which are identical there: a left
    and a right keypoint at (c, y) with equal descriptors have SAD(-k) == SAD(+k), SAD(0) == 0, so
    deltaR == 0, the disparity is exactly 0 and the clamp runs (uRight = uL - 0.01 computed in double).
    Rows 120.. carry accepted matches with SAD > 0, so the median is positive and the clamped ones stay."""
    g = np.random.default_rng(seed)
    L = texture(seed)
    c = 160
    L[:120, c + 1:] = L[:120, c - 1:0:-1][:, :W - c - 1]
    R = shifted(L, 7, seed + 1)
    R[:120] = L[:120]
    b = Builder("clamp", L, R)
    for i in range(10):
        b.pair(g, c, 10 + 10 * i + 0.25 * (i % 4), c, 0, claim="clamp")
    background(b, g, 30, 7, (130, 230))
    return b.scene()


def _sad_block(L, R, xl, xr, y, bright, A=510):
    """Left 11x11 patch at (xl, y): p, its centre row 0.  Right 21x11 strip at (xr, y): 0, its centre
    row q; p + q = A.  Every centred difference a - c = p + q - (strip pixel) is then >= 0 and
    SAD(inc) = 110 A - (sum of the window's off-centre-row pixels): `bright` (strip column offset ->
    value <= A, written above the centre row) steers the eleven SADs."""
    p = min(A, 255)
    q = A - p
    assert 0 <= q <= 255 and all(0 <= v <= min(A, 255) for v in bright.values())
    L[y - 5:y + 6, xl - 5:xl + 6] = p
    L[y, xl - 5:xl + 6] = 0
    R[y - 5:y + 6, xr - 10:xr + 11] = 0
    R[y, xr - 10:xr + 11] = q
    for dx, v in bright.items():
        R[y - 2, xr + dx] = v


def scene_large_sad(seed):
    """Accepted matches whose SADs are all above 32767 (56100 - 2 v): bright pixels at strip columns -5
    and +5 make inc = 0 the unique minimum.  The median filter's radix select works on their high bytes."""
    g = np.random.default_rng(seed)
    L = np.full((H, W), 128, np.uint8)
    R = np.full((H, W), 128, np.uint8)
    b = Builder("large_sad", L, R)
    k = 0
    for yy in (20, 60, 100, 140, 180):
        for xl in (120, 200):
            v = 10 + 12 * k
            _sad_block(L, R, xl, xl - 20, yy, {-5: v, 5: v})
            b.pair(g, xl, yy, xl - 20, 0, claim="ok", uR_near=xl - 20)
            k += 1
    b.L, b.R = L, R
    return b.scene()


def scene_sad_ties(seed):
    """SAD ties, where the first strict minimum wins.  Flat images: all eleven SADs are 0, the winner is
    inc = -5 (edgeinc).  Blocks of scene_large_sad with ONE bright pixel at strip column +3: the windows
    of inc = -2..5 all hold it, SAD(-5..-3) = 56100 > SAD(-2..5) = 56100 - v; the winner is inc = -2, with
    d1 > d2 == d3 and deltaR = 0.5 exactly (a last-minimum rule would take inc = 5: edgeinc)."""
    g = np.random.default_rng(seed)
    L = np.full((H, W), 128, np.uint8)
    R = np.full((H, W), 128, np.uint8)
    b = Builder("sad_ties", L, R)
    for i in range(4):
        b.pair(g, 150 + 10 * i, 200 + 2 * i, 120 + 10 * i, 0, claim="edgeinc")
    for k, yy in enumerate((20, 60, 100, 140)):
        for xl in (120, 220):
            _sad_block(L, R, xl, xl - 20, yy, {3: 40 + 10 * k})
            b.pair(g, xl, yy, xl - 20, 0, claim="ok", uR_near=xl - 20 - 2 + 0.5)
    # a UNIQUE minimum at inc = -5 / +5 (one bright pixel that only that window holds): edgeinc; without
    # the test the parabola through the neighbour would be accepted
    for k, xl in enumerate((60, 120, 180)):
        _sad_block(L, R, xl, xl - 20, 170, {-10: 50 + 10 * k})
        b.pair(g, xl, 170, xl - 20, 0, claim="edgeinc")
        _sad_block(L, R, xl + 100, xl + 80, 185, {10: 50 + 10 * k})
        b.pair(g, xl + 100, 185, xl + 80, 0, claim="edgeinc")
    b.L, b.R = L, R
    return b.scene()


def scene_far_exact(seed):
    """maxD = 20 and blocks of scene_large_sad (deltaR == 0, bestuR == the right keypoint's x exactly): a
    disparity of exactly maxD is refused (far), 19 is accepted.  The candidate sits on uR == minU."""
    g = np.random.default_rng(seed)
    L = np.full((H, W), 128, np.uint8)
    R = np.full((H, W), 128, np.uint8)
    b = Builder("far_exact", L, R, bf=20.0, baseline=1.0)
    for k, yy in enumerate((20, 60, 100, 140)):
        _sad_block(L, R, 100, 80, yy, {-5: 20 + 5 * k, 5: 20 + 5 * k})
        b.pair(g, 100, yy, 80, 0, claim="far")
        _sad_block(L, R, 220, 201, yy, {-5: 30 + 5 * k, 5: 30 + 5 * k})
        b.pair(g, 220, yy, 201, 0, claim="ok", uR_near=201)
    b.L, b.R = L, R
    return b.scene()


def scene_median_edge(seed):
    """The final filter's two comparisons, on SADs set exactly (110 A - 2 v): the accepted set, sorted, is
    3280 x4, 4000, 8398, 8400 x2.  Its size is even, element size / 2 is 4000 (element (size - 1) / 2 is
    3280), and thDist = (1.5f * 1.4f) * 4000 is 8400 exactly in float: 8400 is removed (first < thDist is
    false), 8398 stays."""
    g = np.random.default_rng(seed)
    L = np.full((H, W), 128, np.uint8)
    R = np.full((H, W), 128, np.uint8)
    b = Builder("median_edge", L, R)
    sads, median = {}, {}
    spec = [(30, 10, 3280)] * 4 + [(37, 35, 4000), (77, 36, 8398), (77, 35, 8400), (77, 35, 8400)]
    for k, (A, v, sad) in enumerate(spec):
        xl, yy = 100 + 100 * (k % 2), 20 + 25 * k
        assert 110 * A - 2 * v == sad
        _sad_block(L, R, xl, xl - 20, yy, {-5: v, 5: v}, A)
        i = b.pair(g, xl, yy, xl - 20, 0, claim="ok")
        sads[i], median[i] = sad, sad == 8400
    b.L, b.R = L, R
    out = b.scene()
    out["sad_is"], out["median_is"] = sads, median
    return out


def scene_far_neg(seed):
    """maxD = 4.  Rows 0..79 are shifted by 7: a candidate inside [uL - 4, uL] whose SAD refinement lands
    at disparity 7 >= maxD (far).  Rows 80..159 are shifted the other way (by -3): the refinement lands at
    a negative disparity (neg).  Rows 160.. are shifted by 2: accepted."""
    g = np.random.default_rng(seed)
    L = texture(seed)
    R = shifted(L, 7, seed + 1)
    R[80:160] = shifted(L, -3, seed + 2)[80:160]
    R[160:] = shifted(L, 2, seed + 3)[160:]
    b = Builder("far_neg", L, R, bf=4.0, baseline=1.0)
    for i in range(6):
        uL = 100 + 20 * i + 0.5 * (i % 2)
        b.pair(g, uL, 12 + 10 * i, uL - 3, 0, claim="far")
        b.pair(g, uL, 92 + 10 * i, uL - 1, 0, claim="neg")
        b.pair(g, uL, 172 + 10 * i, uL - 3, 0, claim=ACCEPT)
    return b.scene()


def scene_borders(seed, scale=1.2, nlevels=8):
    """Keypoints within 10 or 11 level-pixels of a border, at every level, placed one float apart where
    the rounding of x * inv_scale decides: the right match at the first x whose scaled position makes
    endu == cols (endu) and at the float below it (the extreme legal strip; with the left patch ending on
    the level's last column, once on the level's bottom legal row); the left patch one column too far
    right (guard); the right match 9 / 10 level-pixels from the left border (guard / legal); the left
    keypoint 4 / 5 level-rows from the top and 5 / 6 from the bottom (guard / legal)."""
    g = np.random.default_rng(seed)
    L = texture(seed)
    R = shifted(L, 7, seed + 1)
    b = Builder("borders_s%g_n%d" % (scale, nlevels), L, R, scale, nlevels)
    sc, _ = lit.scale_factors(scale, nlevels)
    wh = extraction(b.params, L).level_wh
    past_sad_window = PAST_ORB[2:]  # neither endu nor guard
    for l in range(nlevels):
        lw, lh = (int(v) for v in wh[l])
        s = float(sc[l])
        fx = functools.partial(first_x_rounding_to, level=l, scale=scale, nlevels=nlevels)
        rows = [F32((8 + k * (lh - 18) / 6.0) * s) for k in range(6)]  # level rows 8 .. lh - 10
        x_endu, x_last = fx(lw - 11), next_down(fx(lw - 11))
        xl_last, xl_out = next_down(fx(lw - 5)), fx(lw - 5)             # scaled uL == cols - 6 / cols - 5
        b.pair(g, xl_last, rows[0], x_endu, l, claim="endu")
        b.pair(g, xl_last, rows[1], x_last, l, claim=past_sad_window)
        b.pair(g, xl_last, next_down(fx(lh - 5)), x_last, l, claim=past_sad_window)  # bottom-right legal window
        b.pair(g, xl_out, rows[2], x_last, l, claim="guard")
        b.pair(g, 25 * s, rows[3], next_down(fx(10)), l, claim="guard")
        b.pair(g, 25 * s, rows[4], fx(10), l, claim=past_sad_window)
        b.pair(g, 40 * s, next_down(fx(5)), 40 * s - 7, l, claim="guard")
        b.pair(g, 60 * s, fx(5), 60 * s - 7, l, claim=past_sad_window)
        b.pair(g, 40 * s, fx(lh - 5), 40 * s - 7, l, claim="guard")
    return b.scene()


def scene_bands(seed, scale=1.2, nlevels=8):
    """Band limits ceil(y + r) / floor(y - r) of a right keypoint at integer and fractional y: left
    keypoints on rows minr - 1, minr, maxr, maxr + 1; bands cut at rows 0 and nRows - 1; at octave 0 and
    at the top octave."""
    g = np.random.default_rng(seed)
    L = texture(seed)
    R = shifted(L, 7, seed + 1)
    b = Builder("bands_s%g_n%d" % (scale, nlevels), L, R, scale, nlevels)
    sc, _ = lit.scale_factors(scale, nlevels)
    x = 60.0
    for o in sorted({0, nlevels - 1}):
        r = F32(2.0) * sc[o]
        for y in ((20.0, 45.25, 70.5) if o == 0 else (110.0, 150.25, 190.5)):
            y = F32(y)
            maxr, minr = int(np.ceil(y + r)), int(np.floor(y - r))
            d = rand_desc(g)
            b.right(x - 7, y, o, d)
            b.left(x, minr - 0.25, o, d, claim="norow")        # row minr - 1
            b.left(x, float(minr), o, d, claim=PAST_ORB)
            b.left(x, maxr + 0.75, o, d, claim=PAST_ORB)       # row maxr
            b.left(x, float(maxr + 1), o, d, claim="norow")
            x += 45.0
    # cut bands (octave 0 rows 0 and nRows - 1)
    d = rand_desc(g)
    b.right(100.0, 1.5, 0, d)
    b.left(107.0, 0.0, 0, d, claim="guard")
    b.left(107.0, 0.75, 0, d, claim="guard")
    d = rand_desc(g)
    b.right(200.0, H - 1.5, 0, d)
    b.left(207.0, H - 0.5, 0, d, claim="guard")
    b.left(207.0, H - 1.0, 0, d, claim="guard")
    return b.scene()


def scene_filters(seed, scale=1.2, nlevels=8):
    """The candidate filters.  uR == minU and uR == maxU pass, one float step outside each does not; a
    descriptor at Hamming distance 74 passes, at 75 does not; a perfect-descriptor candidate at octave
    levelL +- 2 is ignored (at levelL = 0 and at the top level) while levelL +- 1 is taken."""
    g = np.random.default_rng(seed)
    L = texture(seed)
    R = shifted(L, 7, seed + 1)
    b = Builder("filters_s%g_n%d" % (scale, nlevels), L, R, scale, nlevels)
    maxD = F32(BF) / F32(BASELINE)
    y = 20.0
    for uL in (F32(150.0), F32(200.3), F32(251.77)):
        minU = uL - maxD
        for uR, claim in ((uL, PAST_ORB), (next_up(uL), "orb"), (minU, PAST_ORB), (next_down(minU), "orb")):
            b.pair(g, uL, y, uR, 0, claim=claim)
            y += 8.0
    for k, uL in enumerate((150.0, 180.0, 210.0)):
        d = rand_desc(g)
        bits = [int(v) for v in g.permutation(256)[:75]]
        b.left(uL, y, 0, d, claim=ACCEPT, uR_near=uL - 7)
        b.right(uL - 7 + k - 1, y, 0, flip_bits(d, bits[:74]))
        y += 8.0
        b.left(uL, y, 0, d, claim="orb")
        b.right(uL - 7 + k - 1, y, 0, flip_bits(d, bits))
        y += 8.0
    top = nlevels - 1
    sc, _ = lit.scale_factors(scale, nlevels)
    for levelL, other in ((0, 2), (0, 1), (top, top - 2), (top, top - 1)):
        if other < 0 or other >= nlevels or other == levelL:
            continue
        for uL in (120.0, 170.0, 220.0):
            d = rand_desc(g)
            b.left(uL, y, levelL, d, claim="orb" if abs(other - levelL) == 2 else PAST_ORB)
            b.right(uL - 7, y, other, d)
        y += 4.0 * float(sc[max(levelL, other)]) + 4.0
    assert y < H - 1
    return b.scene()


def scene_hamming_tie(seed):
    """Two candidates at the same Hamming distance.  The reference keeps the lowest iR; here that one (the
    true match, 7 px left) lies in a HIGHER octave or at a LARGER y than the other candidate (30 px left),
    so it comes later in the kernel's (octave, y) order.  The wrong winner refines somewhere else."""
    g = np.random.default_rng(seed)
    L = texture(seed)
    R = shifted(L, 7, seed + 1)
    b = Builder("hamming_tie", L, R)
    y = 20.0
    for k in range(8):
        uL = 120.0 + 20 * k
        d = rand_desc(g)
        bits = [int(v) for v in g.permutation(256)[:20]]
        da, db = flip_bits(d, bits[:10]), flip_bits(d, bits[10:])
        if k % 2 == 0:
            b.right(uL - 7 + (k % 3) - 1, y, 1, da)        # lower iR, higher octave
            b.right(uL - 30, y, 0, db)
        else:
            b.right(uL - 7 + (k % 3) - 1, y + 1.5, 0, da)  # lower iR, larger y
            b.right(uL - 30, y - 1.5, 0, db)
        b.left(uL, y, 0, d, claim=ACCEPT, uR_near=uL - 7)
        y += 12.0
    background(b, g, 20, 7, (130, 230))
    return b.scene()


def scene_counts(seed, nR, nL):
    """nR right keypoints, the winner of every left keypoint at the LAST index (nR - 1); the rest are
    fillers with random descriptors on every row and octave.  nL left keypoints."""
    g = np.random.default_rng(seed)
    L = texture(seed)
    R = shifted(L, 7, seed + 1)
    b = Builder("counts_nR%d_nL%d" % (nR, nL), L, R)
    for _ in range(max(nR - 1, 0)):
        b.right(float(g.integers(0, W)), float(g.integers(0, 4 * H)) * 0.25, int(g.integers(0, 8)), rand_desc(g))
    d = rand_desc(g)
    uL, vL = 180.0, 100.0
    if nR:
        b.right(uL - 7, vL, 0, d)
    for i in range(nL):
        claim = "norow" if nR == 0 else ACCEPT
        b.left(uL + (i % 5) - 2, vL + (i // 5) * 0.5 - 1.0, 0, d, claim=claim)
    return b.scene()


def scene_none_accepted(seed):
    """No accepted match at all: every left keypoint leaves early, the median filter sees an empty set."""
    g = np.random.default_rng(seed)
    L = texture(seed)
    R = texture(seed + 1)
    b = Builder("none_accepted", L, R)
    for i in range(6):
        b.left(100.0 + 10 * i, 50.0 + 5 * i, 0, rand_desc(g), claim="orb")
        b.right(90.0 + 10 * i, 50.0 + 5 * i, 0, rand_desc(g))
    for i in range(3):
        b.left(100.0 + 10 * i, 200.0 + 5 * i, 0, rand_desc(g), claim="norow")
    return b.scene()


@functools.lru_cache(maxsize=None)
def all_scenes():
    out = [scene_background(100, n=40), scene_background(101, n=41, n_heavy=4), scene_clamp(110),
           scene_large_sad(120), scene_sad_ties(130), scene_far_neg(140), scene_hamming_tie(150),
           scene_none_accepted(160), scene_far_exact(161), scene_median_edge(162)]
    for nR, nL in ((0, 1), (1, 15), (2, 16), (4095, 17), (4096, 5)):
        out.append(scene_counts(170 + nL, nR, nL))
    for i, (scale, nlevels) in enumerate(PARAM_SETS):
        out.append(scene_borders(200 + i, scale, nlevels))
        out.append(scene_bands(210 + i, scale, nlevels))
        out.append(scene_filters(220 + i, scale, nlevels))
        if (scale, nlevels) != (1.2, 8):
            out.append(scene_background(230 + i, scale, nlevels, n=24, n_heavy=3))
    names = [s["name"] for s in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def by_name(name):
    return {s["name"]: s for s in all_scenes()}[name]


# ------------------------------------------------------------------ references, computed once
_EXTRACTIONS = {}


def extraction(params, img):
    """The oracle's extraction of img (its pyramid is what the scene's keypoints are matched on)."""
    key = (params, img.shape, img.tobytes())
    if key not in _EXTRACTIONS:
        _EXTRACTIONS[key] = oracle.extract(oracle.params(params[0], params[1], params[2], 20, 7), img)
    return _EXTRACTIONS[key]


def pyramids(scene):
    return extraction(scene["params"], scene["L"]), extraction(scene["params"], scene["R"])


def levels(ex, nlevels):
    return [ex.level(l) for l in range(nlevels)]


_LITERAL, _ORACLE = {}, {}


def literal_result(scene):
    if scene["name"] not in _LITERAL:
        exL, exR = pyramids(scene)
        n = scene["params"][2]
        _LITERAL[scene["name"]] = lit.compute_stereo_matches(scene["params"][1], n, scene["kL"], scene["dL"],
                                                             scene["kR"], scene["dR"], levels(exL, n), levels(exR, n),
                                                             scene["bf"], scene["baseline"])
    return _LITERAL[scene["name"]]


def oracle_result(scene):
    """(uRight, depth, sad, nmatches) of oracle_stereo_match on the scene's injected keypoints."""
    if scene["name"] not in _ORACLE:
        exL, exR = pyramids(scene)
        p = oracle.params(scene["params"][0], scene["params"][1], scene["params"][2], 20, 7)
        inL = oracle.Extraction(scene["kL"], scene["dL"], exL.pyramid_flat, exL.level_wh)
        inR = oracle.Extraction(scene["kR"], scene["dR"], exR.pyramid_flat, exR.level_wh)
        _ORACLE[scene["name"]] = oracle.stereo_match(p, inL, inR, scene["bf"], scene["baseline"], with_sad=True)
    return _ORACLE[scene["name"]]

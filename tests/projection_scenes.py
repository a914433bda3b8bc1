"""Crafted SearchByProjection scenes: small frames and MapPoints that put a point on every exit and
boundary of the SearchByProjection family (tests/test_projection_scenes.py).

The rule that makes a scene discriminate: every claimed point has a feature of its own in an otherwise
empty spot, carrying the point's descriptor (or one a stated number of bits away), so a pass ends in a
match to that feature and a fail in -1; every boundary is a pair or triple of points whose compared
value sits on the boundary and one float step off it, with different outcomes.  The inputs that produce
such a value are searched for with the literal (projection_literal), never assumed.

A scene is a dict: name, kind, fr, pts (synth.projection_frame / projection_points layout), kw (th and the
other arguments of the call), claims (point -> dict(exit[, match][, tally])), sweeps (the number of
sweeps py_sweeps must report), host (False where the host call refuses the input: out-of-pyramid levels
reach the kernels only through the device batch).  BY_SIM3 scenes are one direction of SearchBySim3:
fr is the KeyFrame searched in, fr["Tcw"] the pose of the points' own KeyFrame, kw["last_Tcw"] = [sR | t].
"""
import functools
import math

import numpy as np

import oracle
import projection_literal as lit
from projection_literal import BY_SIM3, FUSE, FUSE_SIM3, KEYFRAME, LAST_FRAME, LOCAL, SIM3

F32 = np.float32
KP = oracle.KEYPOINT_DTYPE
W, H = 640, 480
FX = FY = F32(200.0)
CX, CY = F32(320.5), F32(240.25)
BF = F32(40.0)
PYRAMIDS = ((1.2, 8), (1.5, 4), (1.1, 12), (1.2, 1), (1.1, 16))
IMAGE_FAMILY = (FUSE, SIM3, FUSE_SIM3, BY_SIM3)   # KeyFrame::IsInImage: u >= min && u < max
ALL_KINDS = (LOCAL, LAST_FRAME, KEYFRAME, FUSE, SIM3, FUSE_SIM3, BY_SIM3)
TH = {LOCAL: 1.0, LAST_FRAME: 3.0, KEYFRAME: 3.0, FUSE: 3.0, SIM3: 3.0, FUSE_SIM3: 3.0, BY_SIM3: 3.0}
THRESHOLD = {LOCAL: 100, LAST_FRAME: 100, FUSE: 50, SIM3: 50, FUSE_SIM3: 50, BY_SIM3: 100}


def next_up(x):
    return F32(np.nextafter(F32(x), F32(np.inf)))


def next_down(x):
    return F32(np.nextafter(F32(x), F32(-np.inf)))


def steps(x, n):
    for _ in range(abs(n)):
        x = next_up(x) if n > 0 else next_down(x)
    return F32(x)


def flip_bits(d, bits):
    """d with the listed bit positions (0..255) flipped: Hamming distance len(bits) from d."""
    out = np.array(d, np.uint8).copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def scan(x0, value, want, reach=4000):
    """The float32 x nearest x0 with value(x) == want, walking outwards float by float."""
    up = down = F32(x0)
    for _ in range(reach):
        for x in (up, down):
            if value(x) == want:
                return F32(x)
        up, down = next_up(up), next_down(down)
    raise AssertionError("no input within %d floats of %r gives %r" % (reach, x0, want))


def around(x0, value, want, reach=4000):
    """(below, at, above): inputs next to each other whose values are the nearest attainable one below
    `want`, `want` itself and the nearest attainable one above (value is monotone rising in x).  Where a
    sum cancels, the values an input can produce are coarser than the floats near `want`: the step taken
    is the smallest one any input produces."""
    at = lo = hi = scan(x0, value, want, reach)
    while value(lo) == want:
        lo = next_down(lo)
    while value(hi) == want:
        hi = next_up(hi)
    assert value(lo) < want < value(hi)
    return lo, at, hi


def scale_table(scale, nlevels):
    s = [F32(1.0)]
    for _ in range(1, nlevels):
        s.append(F32(np.float64(s[-1]) * scale))
    return np.array(s, np.float32)


def make_frame(scale=1.2, nlevels=8, bounds="frame"):
    """An empty frame.  bounds: "plain" (0..W, 0..H), "frame" (a distorted camera's Frame: fractional
    float bounds, the grid built from them) or "kf" (a KeyFrame of that Frame: the bounds truncated to
    ints for IsInImage and the search window, the grid still from the float bounds)."""
    x0, x1, y0, y1 = F32(0), F32(W), F32(0), F32(H)
    if bounds != "plain":
        x0, x1, y0, y1 = F32(-1.625), F32(W + 0.375), F32(2.6875), F32(H - 0.46875)
    fr = dict(min_x=x0, max_x=x1, min_y=y0, max_y=y1, grid_inv_w=F32(F32(64) / F32(x1 - x0)),
              grid_inv_h=F32(F32(48) / F32(y1 - y0)), nlevels=nlevels, scale_factors=scale_table(scale, nlevels),
              log_scale_factor=F32(np.log(F32(scale))), fx=FX, fy=FY, cx=CX, cy=CY, bf=BF, b=F32(BF / FX),
              Tcw=np.eye(4, dtype=np.float32))
    if bounds == "kf":
        fr.update(grid_min_x=x0, grid_min_y=y0, min_x=F32(int(x0)), min_y=F32(int(y0)), max_x=F32(int(x1)),
                  max_y=F32(int(y1)))
    return fr


class Builder:
    def __init__(self, name, kind, scale=1.2, nlevels=8, bounds=None, seed=0, u_right=True, **kw):
        self.name, self.kind = name, kind
        if bounds is None:
            bounds = "kf" if kind in IMAGE_FAMILY else "frame"
        self.fr = make_frame(scale, nlevels, bounds)
        self.kw = dict(th=TH[kind])
        if kind == LOCAL:
            self.kw["nnratio"] = 0.8
        if kind == LAST_FRAME:
            self.kw.update(last_Tcw=np.eye(4, dtype=np.float32), mono=False)
        if kind == BY_SIM3:
            self.kw["last_Tcw"] = np.eye(4, dtype=np.float32)
        self.kw.update(kw)
        self.g = np.random.default_rng(seed + 1000 * kind)
        self.has_ur = u_right
        self.feats, self.fdesc, self.fur, self.focc = [], [], [], []
        self.p = dict(desc=[], flags=[], pos=[], normal=[], dist_minmax=[], angle=[], octave=[], track=[],
                      track_level=[])
        self.claims, self.sweeps, self.host, self._spot = {}, None, True, 0
        self.pairs = []

    # ---- the frame's features
    def feature(self, x, y, octave, desc, ur=-1.0, occ=0, angle=0.0):
        self.feats.append((F32(x), F32(y), int(octave), F32(angle)))
        self.fdesc.append(np.asarray(desc, np.uint8))
        self.fur.append(F32(ur))
        self.focc.append(int(occ))
        return len(self.feats) - 1

    def frame(self, feats=True):
        k = np.zeros(len(self.feats) if feats else 0, KP)
        for i in range(len(k)):
            k[i]["x"], k[i]["y"], k[i]["octave"], k[i]["angle"] = self.feats[i]
            k[i]["size"], k[i]["response"], k[i]["class_id"] = 31.0, 1.0, -1
        n = len(k)
        fr = dict(self.fr, keys_un=k, desc=np.array(self.fdesc[:n], np.uint8).reshape(-1, 32),
                  occ=np.array(self.focc[:n], np.int8))
        fr["u_right"] = np.array(self.fur[:n], np.float32) if self.has_ur else None
        return fr

    # ---- the MapPoints
    def desc(self):
        return self.g.integers(0, 256, 32, dtype=np.uint8)

    def spot(self):
        """The next empty spot of a 40-pixel lattice (search radii here stay below 15 pixels)."""
        i = self._spot
        self._spot += 1
        assert i < 14 * 10, self.name
        return 60.0 + 40.0 * (i % 14), 60.0 + 40.0 * (i // 14)

    def raw_point(self, pos=(0, 0, 1), normal=(0, 0, 1), dmin=0.0, dmax=1.0, flags=3, angle=0.0, octave=0,
                  track=(0, 0, 0, 0), level=0, desc=None):
        p = self.p
        p["desc"].append(self.desc() if desc is None else np.asarray(desc, np.uint8))
        p["flags"].append(flags)
        p["pos"].append(np.array(pos, np.float32))
        p["normal"].append(np.array(normal, np.float32))
        p["dist_minmax"].append((F32(dmin), F32(dmax)))
        p["angle"].append(F32(angle))
        p["octave"].append(int(octave))
        p["track"].append(np.array(track, np.float32))
        p["track_level"].append(int(level))
        return len(p["desc"]) - 1

    def world(self, pc):
        """The world point whose camera coordinates (in the searched frame) are pc, as float32."""
        T = np.asarray(self.fr["Tcw"], np.float64)
        if self.kind in (SIM3, FUSE_SIM3):
            T = np.asarray(lit.sim3_decompose(self.fr["Tcw"]), np.float64)
        return ((np.asarray(pc, np.float64) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)

    def at(self, u=None, v=None, z=4.0, level=0, **over):
        """A point projecting near (u, v) (default: the next empty spot) at depth z whose distance bounds
        predict `level`, its normal along the viewing ray.  Local non-frustum: the track fields."""
        if u is None:
            u, v = self.spot()
        if self.kind == LOCAL and not self.kw.get("frustum"):
            tr = over.pop("track", (u, v, u - float(BF) / z, 0.5))
            return self.raw_point(track=tr, level=level, **over)
        pc = np.array([(u - float(CX)) * z / float(FX), (v - float(CY)) * z / float(FY), z])
        X = self.world(pc)
        T = lit.sim3_decompose(self.fr["Tcw"]) if self.kind in (SIM3, FUSE_SIM3) else self.fr["Tcw"]
        d = float(np.linalg.norm(pc)) if self.kind == BY_SIM3 else float(
            np.linalg.norm(X.astype(np.float64) - np.array(lit._centre(np.asarray(T, np.float32)), np.float64)))
        sc = float(np.exp(float(self.fr["log_scale_factor"])))
        dmax = d * sc ** (level - 0.5) if level > 0 else d * max(sc ** -0.5, 0.9)  # within 1.2 * dmax
        Ow = np.array(lit._centre(np.asarray(T, np.float32)), np.float64)
        n = (X.astype(np.float64) - Ow) / max(d, 1e-30)
        args = dict(pos=X, normal=n, dmin=dmax / 100.0, dmax=dmax, octave=level)
        args.update(over)
        return self.raw_point(**args)

    def points(self):
        p = self.p
        n = len(p["desc"])
        out = dict(desc=np.array(p["desc"], np.uint8).reshape(n, 32), flags=np.array(p["flags"], np.uint8),
                   pos=np.array(p["pos"], np.float32).reshape(n, 3),
                   normal=np.array(p["normal"], np.float32).reshape(n, 3),
                   dist_minmax=np.array(p["dist_minmax"], np.float32).reshape(n, 2),
                   angle=np.array(p["angle"], np.float32), octave=np.array(p["octave"], np.int32))
        if self.kind == LOCAL:
            out["track"] = np.array(p["track"], np.float32).reshape(n, 4)
            out["track_level"] = np.array(p["track_level"], np.int32)
        return out

    def search(self, feats=False):
        kw = dict(self.kw)
        kw["limit"] = kw.pop("view_cos_limit", 0.5)
        return lit.Search(self.frame(feats), self.points(), self.kind, **kw)

    def uv(self, pos):
        """(u, v) of a world point as this problem's kind forms them (the literal's arithmetic)."""
        one = dict(desc=np.zeros((1, 32), np.uint8), flags=np.ones(1, np.uint8), pos=np.array([pos], np.float32))
        kw = {k: v for k, v in self.kw.items() if k in ("last_Tcw", "mono", "frustum")}
        if self.kind == LOCAL:
            one.update(normal=np.zeros((1, 3), np.float32), dist_minmax=np.array([[0, -1]], np.float32))
        code, u, v, _, _ = lit.Search(self.frame(False), one, self.kind, self.kw["th"], **kw).uv(0)
        assert code is None, code
        return u, v

    def probe(self, i):
        """Point i's query (centre, radius, level window ...) or its exit code, by the literal."""
        return self.search().query(i)

    def own(self, i, dx=0.0, dy=0.0, bits=0, octave=None, **kw):
        """A feature for point i at its projection (+ dx, dy), on its predicted level, `bits` bits away."""
        q = self.probe(i)
        if isinstance(q, str):  # a rejected point: its feature still sits at its projection
            u, v = self.uv(self.p["pos"][i])
            q = dict(x=u, y=v, level=0)
        lv = q["level"] if octave is None else octave
        return self.feature(F32(q["x"]) + F32(dx), F32(q["y"]) + F32(dy), lv,
                            flip_bits(self.p["desc"][i], range(bits)), **kw)

    def claim(self, i, exit, match=None, tally=None):
        c = dict(exit=exit)
        if match is not None or exit not in ("matched", "matched_then_rotated_out"):
            c["match"] = -1 if match is None else match
        if tally is not None:
            c["tally"] = dict(tally)
        self.claims[i] = c

    def pair(self, i, j):
        """Points i and j sit on the two sides of one boundary: their outcomes must differ."""
        self.pairs.append((i, j))

    def positions(self, i):
        """feature -> (grid column, position within that column's part of point i's window), in the
        reference's enumeration order.  The kernels give position p of a column to lane p % 16 of the
        point's 16-lane group."""
        F = lit.PyFrame(self.frame())
        q = self.search(True).query(i)
        x0, x1, y0, y1 = F.cell_range(q["x"], q["y"], q["r"])
        out = {}
        for ix in range(x0, x1 + 1):
            p = 0
            for iy in range(y0, y1 + 1):
                for j in F.grid[ix][iy]:
                    out[j] = (ix, p)
                    p += 1
        return out

    def apart(self, i, f0, f1):
        """How many enumeration positions lie between features f0 and f1 of point i's window; they must
        share a grid column."""
        pos = self.positions(i)
        assert pos[f0][0] == pos[f1][0], (self.name, i, pos[f0], pos[f1])
        return pos[f1][1] - pos[f0][1]

    def matched(self, i, **kw):
        """Point i with a feature of its own, claimed to match it."""
        f = self.own(i, **kw)
        self.claim(i, "matched", f)
        return f

    def scene(self):
        fuse = self.kind in (FUSE, FUSE_SIM3, BY_SIM3)
        n = len(self.p["desc"])
        sweeps = self.sweeps if self.sweeps is not None else (1 if fuse or n == 0 else 2)
        return dict(name=self.name, kind=self.kind, fr=self.frame(), pts=self.points(), kw=dict(self.kw),
                    claims=dict(self.claims), sweeps=sweeps, host=self.host, pairs=tuple(self.pairs))


def kname(kind, frustum=False):
    return lit.KIND_NAMES[kind] + ("_frustum" if frustum else "")


def variants():
    """(kind, extra kw) for every way the family runs: the seven kinds, the local kind also with the
    frustum fused in front."""
    return [(k, {}) for k in ALL_KINDS] + [(LOCAL, dict(frustum=True))]


# ------------------------------------------------------------------ projection: depth
def scene_depth(kind, kw):
    """c[2] negative, -0.0, +0.0 with c[0] != 0 (infinite u), +0.0 with c[0] == c[1] == 0 (NaN), the smallest
    positive normal (projects onto the principal point), and an ordinary point.  The -0.0 reaches the depth
    test as -0.0 under the frustum, the last-frame, keyframe and Fuse kinds only: the Sim3 decomposition
    adds +0.0f to every entry of the pose and SearchBySim3's second transform adds t = +0.0, so under
    those three kinds the same point arrives as +0.0 (with the same outcome)."""
    b = Builder("depth_" + kname(kind, kw.get("frustum")), kind, **kw)
    b.fr["Tcw"][2, 3] = F32(-0.0)  # so that a row of -0.0 products keeps its sign through `+ t`
    tiny = np.finfo(np.float32).tiny
    i = b.raw_point(pos=(0, 0, tiny), dmin=0.0, dmax=F32(tiny) * F32(1.1))
    b.matched(i)
    i = b.at()
    b.matched(i)
    # behind the camera, the projection inside the image: only the keyframe kind has no depth test
    u, v = b.spot()
    z = -4.0
    X = ((u - float(CX)) * z / float(FX), (v - float(CY)) * z / float(FY), z)
    d = float(np.linalg.norm(X))
    i = b.raw_point(pos=X, normal=np.array(X) / d, dmin=d / 100, dmax=d / math.sqrt(1.2))
    if kind == KEYFRAME:
        q = b.probe(i)
        b.claim(i, "matched", b.feature(q["x"], q["y"], 0, b.p["desc"][i]))
    else:
        b.feature(u, v, 0, b.p["desc"][i])
        b.claim(i, "behind")
    i = b.raw_point(pos=(-1, -1, -0.0))      # c = (-1, -1, -0.0): invz = -inf, u = +inf
    b.claim(i, "behind" if kind == LAST_FRAME else "out_of_image")
    i = b.raw_point(pos=(1, 1, 0.0))         # u = v = +inf
    b.claim(i, "out_of_image")
    i = b.raw_point(pos=(0, 0, 0.0))         # 0 * inf
    b.claim(i, "out_of_image" if kind in IMAGE_FAMILY else "nan_uv")
    i = b.raw_point(pos=(1, 0, 0.0), flags=0)
    b.claim(i, "flag_off")
    return b.scene()


# ------------------------------------------------------------------ projection: image bounds
def scene_bounds(kind, kw):
    """u and v exactly on min_x / max_x / min_y / max_y and one step either side, each point with a
    feature of its own 6 pixels inside the image (5 would round into grid column 64).  The last-frame,
    keyframe and frustum tests keep u == max; KeyFrame::IsInImage rejects it.  fx * x skips some floats,
    so the depth is searched too until some x lands u on the bound."""
    b = Builder("bounds_" + kname(kind, kw.get("frustum")), kind, th=9.0, **kw)
    strict_max = kind in IMAGE_FAMILY
    k = 0
    for axis, side in (("x", "min"), ("x", "max"), ("y", "min"), ("y", "max")):
        want = F32(b.fr[side + "_" + axis])
        other = 100.0 + 100.0 * k  # the other coordinate: the three points of a bound share no window
        k += 1
        for z in (1.0, 3.0, 5.0, 7.0, 1.5, 2.5, 6.0, 9.0, 11.0, 13.0):
            if axis == "x":
                place = lambda c, off, z=z: (c, (other + 45.0 * off - float(CY)) * z / float(FY), z)  # noqa: E731
                guess, value = (float(want) - float(CX)) * z / float(FX), lambda c: b.uv(place(c, 0))[0]  # noqa: E731
            else:
                place = lambda c, off, z=z: ((other + 45.0 * off - float(CX)) * z / float(FX), c, z)  # noqa: E731
                guess, value = (float(want) - float(CY)) * z / float(FY), lambda c: b.uv(place(c, 0))[1]  # noqa: E731
            try:
                cs = around(guess, value, want, 60)
                break
            except AssertionError:
                continue
        else:
            raise AssertionError((b.name, axis, side))
        trio = []
        for off, c in zip((-1, 0, 1), cs):
            pos = place(c, off)
            d = float(np.linalg.norm(pos))
            # level 7: Fuse's gate then lets a feature 6 pixels away through
            i = b.raw_point(pos=pos, normal=np.array(pos) / d, dmin=d / 100, dmax=d * 1.2 ** 6.5, octave=7)
            if side == "min":
                inside = off >= 0
            else:
                inside = off < 0 if strict_max else off <= 0
            uu, vv = b.uv(pos)  # the feature sits where its own point projects in the free coordinate
            u, v = (float(want), float(vv)) if axis == "x" else (float(uu), float(want))
            inward = 6.0 if side == "min" else -6.0
            f = b.feature(u + (inward if axis == "x" else 0.0), v + (inward if axis == "y" else 0.0), 7,
                          b.p["desc"][i])
            b.claim(i, "matched", f) if inside else b.claim(i, "out_of_image")
            trio.append(i)
        b.pair(trio[0], trio[1]) if side == "min" or strict_max else b.pair(trio[1], trio[2])
    return b.scene()


# ------------------------------------------------------------------ distance, normal, viewing cosine
def scene_distance(kind, kw):
    """d3 == 0.8f*dmin and d3 == 1.2f*dmax exactly (kept) and the bound one float past d3 (rejected); for
    Fuse and the Sim3 kinds dot == 0.5*d3 exactly and one float of the normal below; for the frustum the
    viewing cosine == the limit exactly and one float below it."""
    b = Builder("distance_" + kname(kind, kw.get("frustum")), kind, **kw)
    for which in ("min", "max"):
        factor = F32(0.8) if which == "min" else F32(1.2)
        two = []
        for out in (False, True):
            i = b.at(level=0)
            d3 = b.search().d3(i)
            want = d3 if not out else (next_up(d3) if which == "min" else next_down(d3))
            m = scan(float(d3) / float(factor), lambda m: F32(factor * m), want)
            f = b.own(i)
            b.p["dist_minmax"][i] = (m, b.p["dist_minmax"][i][1]) if which == "min" else (F32(0.0), m)
            b.claim(i, "distance") if out else b.claim(i, "matched", f)
            two.append(i)
        b.pair(*two)
    if kind in (FUSE, SIM3, FUSE_SIM3) or kw.get("frustum"):
        # PO = (+-1, +-4, 8) / 2 has the exact norm 4.5, so dot = 8/2 * nz == 0.5 * 4.5 at nz = 0.5625
        two = []
        for sx, nz in ((1, F32(0.5625)), (-1, next_down(0.5625))):
            i = b.raw_point(pos=(0.5 * sx, 2.0, 4.0), normal=(0, 0, nz), dmin=0.0, dmax=4.5 / math.sqrt(1.2))
            two.append(i)
            if nz == F32(0.5625):
                b.matched(i)
            elif kw.get("frustum"):
                b.own(i)
                vc = F32(np.float64(4.0 * float(nz)) / np.float64(4.5))
                assert vc < F32(0.5)
                b.claim(i, "view_cos")
            else:
                b.own(i)
                b.claim(i, "normal")
        b.pair(*two)
    if kw.get("frustum"):  # exactly one float below the limit: a small x component tunes the double dot
        want = next_down(0.5)
        nx = scan(2.7e-7, lambda nx: F32(np.float64(-0.5 * float(nx) + 4.0 * 0.5625) / np.float64(4.5)), want, 20000)
        i = b.raw_point(pos=(-0.5, -2.0, 4.0), normal=(nx, 0, 0.5625), dmin=0.0, dmax=4.5 / math.sqrt(1.2))
        b.own(i)
        b.claim(i, "view_cos")
        b.pair(two[0], i)
    return b.scene()


# ------------------------------------------------------------------ PredictScale
def scene_predict(kind, kw, scale=1.2, nlevels=8):
    """log(dmax/dist)/log(scaleFactor) an exact integer L (ceil: L) and the next value above it (ceil: L + 1),
    each point with a feature on octave L - 1, which only the first window holds; a quotient below 0 and
    one above the top level, clamped; the level-0 window (min_level -1) finding an octave-0 feature."""
    b = Builder("predict_%s_s%g_n%d" % (kname(kind, kw.get("frustum")), scale, nlevels), kind, scale, nlevels, **kw)
    logsf = b.fr["log_scale_factor"]
    found = 0
    for L in range(1, nlevels - 1):
        pair = []
        for _ in range(2):
            i = b.at(level=L)
            d3 = b.search().d3(i)
            try:
                pair.append((i,) + around(float(d3) * float(b.fr["scale_factors"][L]),
                                          lambda m: lit.predict_quotient(m, d3, logsf), F32(L), 400))
            except AssertionError:
                break
        if len(pair) < 2:
            for _ in range(len(pair) + 1):
                for key in b.p:
                    b.p[key].pop()
                b._spot -= 1
            continue
        (i, _, at, _), (j, _, _, hi) = pair
        b.p["dist_minmax"][i] = (F32(at / 100), at)
        assert b.probe(i)["level"] == L
        b.matched(i, octave=L - 1)
        b.p["dist_minmax"][j] = (F32(hi / 100), hi)
        assert b.probe(j)["level"] == L + 1
        b.own(j, octave=L - 1)
        b.claim(j, "no_candidate", tally=dict(level=1))
        b.pair(i, j)
        found += 1
        if found == 2:
            break
    assert found or nlevels <= 2, b.name
    i = b.at(level=0)           # quotient -0.5: clamped to level 0, whose window is octaves -1..0
    assert lit.predict_quotient(b.p["dist_minmax"][i][1], b.search().d3(i), logsf) < 0
    b.matched(i, octave=0)
    i = b.at(level=nlevels + 3)  # clamped to the top level
    b.matched(i, octave=nlevels - 1)
    if nlevels > 1:
        i = b.at(level=nlevels + 3)
        b.own(i, octave=0)
        b.claim(i, "no_candidate", tally=dict(level=1))
    return b.scene()


# ------------------------------------------------------------------ the local kind on given track fields
def scene_local(th):
    """RadiusByViewingCos at 0.998 and one float above; th == 1 (no multiply) or not; |dx| == r, |dy| == r
    and one float inside; the uR test at |ur - uR| == r and one float above, uR = -1, 0, the smallest
    positive floats; windows outside the grid; features that round out of the grid; the ratio test."""
    b = Builder("local_th%g" % th, LOCAL, th=th)
    r4, r25 = F32(F32(4.0) * F32(th)) if th != 1 else F32(4.0), F32(F32(2.5) * F32(th)) if th != 1 else F32(2.5)
    mid = float(r4 + r25) / 2

    def pt(u, v, vc=0.5, ur=50.0, level=0, **kw):
        return b.raw_point(track=(u, v, ur, vc), level=level, **kw)

    b.pair(0, 1)  # view cosine 0.998 and one float above
    for vc, ok in ((F32(0.998), True), (next_up(0.998), False), (next_down(0.998), True)):
        u, v = b.spot()
        i = pt(u, v, vc)
        f = b.feature(u + mid, v, 0, b.p["desc"][i])
        b.claim(i, "matched", f) if ok else b.claim(i, "no_candidate", tally=dict(radius=1))
    for axis in (0, 1):
        for inside in (False, True):
            u, v = b.spot()
            i = pt(u, v)
            k = F32((u if axis == 0 else v) + float(r4))
            assert F32(k - F32(u if axis == 0 else v)) == r4
            if inside:
                k = next_down(k)
            f = b.feature(k if axis == 0 else u, v if axis == 0 else k, 0, b.p["desc"][i])
            b.claim(i, "matched", f) if inside else b.claim(i, "no_candidate", tally=dict(radius=1))
            if inside:
                b.pair(i - 1, i)
    n0 = len(b.p["desc"])
    b.pair(n0, n0 + 1)      # |ur - uR| == r and one float above
    b.pair(n0 + 3, n0 + 4)  # uR == 0 and the smallest positive float
    tiny, sub = np.finfo(np.float32).tiny, np.nextafter(F32(0), F32(1))
    for ur, ok in ((F32(50.0) - r4, True), (next_down(F32(50.0) - r4), False), (-1.0, True), (0.0, True),
                   (sub, False), (tiny, False)):
        u, v = b.spot()
        i = pt(u, v)
        f = b.feature(u + 1.0, v, 0, b.p["desc"][i], ur=ur)
        b.claim(i, "matched", f) if ok else b.claim(i, "no_candidate", tally=dict(ur=1))
    # windows outside the grid, and features whose cell is outside it (never enumerated)
    for u, v in ((-60.0, 100.0), (W + 60.0, 100.0), (100.0, -60.0), (100.0, H + 60.0)):
        i = pt(u, v)
        b.feature(u + 1.0, v, 0, b.p["desc"][i])
        b.claim(i, "no_candidate", tally=dict(radius=0))
    for (u, v), (fx_, fy_) in (((-6.0, 300.0), (-8.0, 300.0)), ((636.0, 300.0), (637.5, 300.0)),
                               ((300.0, 476.0), (300.0, 477.5)), ((400.0, 1.0), (400.0, -3.0))):
        i = pt(u, v)
        f = b.feature(fx_, fy_, 0, b.p["desc"][i])
        g = lit.PyFrame(b.frame()).grid
        assert not any(f in cell for col in g for cell in col), (b.name, fx_, fy_)
        b.claim(i, "no_candidate", tally=dict(radius=0))
    # windows that start left of column 0 / end right of column 63 and still hold their feature
    for u, v in ((1.0, 200.0), (634.0, 200.0), (200.0, 4.0), (250.0, 472.0)):
        i = pt(u, v)
        b.claim(i, "matched", b.feature(u + (1.5 if u < 300 else -1.5), v + (1.5 if v < 200 else -1.5), 0,
                                        b.p["desc"][i]))
    # the ratio test, nnratio 0.8: 0.8f * 50 == 40 in float
    assert F32(F32(0.8) * F32(50)) == F32(40)

    def cands(level, spec, filler=0):
        """A point over the features of spec (bits away, octave), `filler` far features (90+ bits) after
        the first: with 15 of them the first two of spec are 16 enumeration positions apart, which the
        kernels hand to one lane of the point's 16-lane group (best and second best from one lane)."""
        u, v = b.spot()
        i = pt(u, v, level=level)
        d = b.p["desc"][i]
        ids = []
        for k, (bits, lv) in enumerate(spec):
            ids.append(b.feature(u + 0.5 * k - 0.5, v, lv, flip_bits(d, range(bits))))
            if k == 0:
                for m in range(filler):
                    b.feature(u + 0.1 * (m % 5), v + 0.1 * (m // 5), level, flip_bits(d, range(60, 150 + m)))
        if filler:
            assert b.apart(i, ids[0], ids[1]) == filler + 1, b.name
        return i, ids

    for filler in (0, 15, 31):  # adjacent lanes; 16 and 32 positions apart: the same lane
        for d1, code in ((40, "matched"), (41, "ratio"), (39, "matched")):
            i, ids = cands(2, [(50, 2), (d1, 2)], filler)   # the second best enumerated before the best
            b.claim(i, code, ids[1] if code == "matched" else None)
            j, ids = cands(2, [(d1, 2), (50, 2)], filler)   # and after it
            b.claim(j, code, ids[0] if code == "matched" else None)
            if d1 == 41:
                b.pair(i - 2, i)
                b.pair(j - 2, j)
    i, ids = cands(2, [(45, 2), (50, 1)])              # the second best on another level
    b.claim(i, "matched", ids[0])
    i, ids = cands(2, [(45, 2)])                       # no second candidate
    b.claim(i, "matched", ids[0])
    i, ids = cands(2, [(60, 1), (50, 2), (41, 2)])
    b.claim(i, "ratio")
    i, ids = cands(2, [(41, 2), (45, 1), (50, 2)])
    b.claim(i, "matched", ids[0])
    i, ids = cands(2, [(100, 2)])
    b.claim(i, "matched", ids[0])
    i, ids = cands(2, [(101, 2)])
    b.claim(i, "over_threshold")
    i, ids = cands(2, [(0, 2), (0, 3)])                # octave 3 is outside the window 1..2
    b.claim(i, "matched", ids[0], tally=dict(level=1))
    i = pt(*b.spot(), flags=2)
    b.claim(i, "flag_off")
    return b.scene()


def scene_cell_edges():
    """Plain bounds (0..640, cells of 10 pixels, 64/640 = 0.1f): windows whose floor / ceil land exactly on
    a cell edge, each with its feature in the first / last cell of the range."""
    b = Builder("local_cell_edges", LOCAL, bounds="plain")
    F = lit.PyFrame(b.frame(False))
    for (u, v), (du, dv), edge in (((94.0, 200.0), (-3.5, 0.0), (9, None)), ((96.0, 250.0), (3.9, 0.0), (None, 10)),
                                   ((300.0, 94.0), (0.0, -3.5), (9, None)), ((350.0, 96.0), (0.0, 3.9), (None, 10))):
        i = b.raw_point(track=(u, v, 50.0, 0.5), level=0)
        x0, x1, y0, y1 = F.cell_range(u, v, 4.0)
        lo, hi = (x0, x1) if du else (y0, y1)
        assert (edge[0] is None or lo == edge[0]) and (edge[1] is None or hi == edge[1]), (u, v, x0, x1, y0, y1)
        f = b.feature(u + du, v + dv, 0, b.p["desc"][i])
        b.claim(i, "matched", f)
    g = lit.PyFrame(b.frame()).grid
    assert 0 in g[9][20] and 1 in g[10][25] and 2 in g[30][9] and 3 in g[35][10]
    return b.scene()


def scene_out_of_pyramid(kind):
    """A local point whose track level, or a last-frame point whose octave, lies outside the pyramid: the
    host call refuses it, the device batch reaches the kernels' guard."""
    b = Builder("out_of_pyramid_" + kname(kind), kind)
    b.host = False
    for lv in (-1, 8, 3):
        i = b.at(level=3)
        b.own(i, octave=3)
        b.p["track_level"][i] = b.p["octave"][i] = lv
        if lv == 3:
            b.claim(i, "matched", len(b.feats) - 1)
        else:
            b.claim(i, "level_unset" if kind == LOCAL else "octave_range")
    return b.scene()


# ------------------------------------------------------------------ the last-frame kind's level windows
LAST_FRAME_MODES = {"at_b": (0, False), "above_b": (1, False), "below_b": (-1, False), "at_minus_b": (0, False),
                    "below_minus_b": (-1, False), "above_minus_b": (1, False), "mono_far": (None, True)}


def scene_last_frame_levels(mode):
    """tlc.z == b exactly (neither direction), one float either side, both signs, and bMono with a large
    tlc.z; points on octave 0, 3 and the top one, each over features whose octaves tell the three level
    windows apart (forward at octave 0 is min 0, max -1: no level check at all)."""
    off, mono = LAST_FRAME_MODES[mode]
    b = Builder("last_frame_levels_" + mode, LAST_FRAME, mono=mono)
    bb = F32(b.fr["b"])
    tz = F32(10.0) if off is None else (steps(-bb, off) if "minus" in mode else steps(bb, off))
    b.kw["last_Tcw"] = np.eye(4, dtype=np.float32)
    b.kw["last_Tcw"][2, 3] = tz  # Tcw = I: twc = 0 and tlc.z = the last pose's t.z
    direction = "sym" if mono or abs(tz) <= bb else ("fwd" if tz > 0 else "bwd")
    table = {0: ((2, "fwd"), (1, "sym"), (0, "bwd")), 3: ((1, "bwd"), (2, "sym"), (5, "fwd"), (3, None)),
             7: ((5, "bwd"), (6, "sym"), (7, "fwd"))}
    for o, feats in table.items():
        i = b.at(octave=o)
        ids = {}
        for bits, (octave, who) in enumerate(feats):
            ids[who] = b.own(i, dx=0.5 * bits, bits=bits, octave=octave)
        b.claim(i, "matched", ids[direction])
    s = b.search()
    assert (s.fwd, s.bwd) == (direction == "fwd", direction == "bwd"), (mode, s.tlc, bb)
    return b.scene()


# ------------------------------------------------------------------ occupancy and blocking
def scene_occupancy(kind, kw):
    """occ 0 / 1 / 2 on a point's own feature; an earlier point without and with observations (flags bit
    1) on the feature of a later one."""
    b = Builder("occupancy_" + kname(kind, kw.get("frustum")), kind, **kw)
    kf, fuse = kind in (KEYFRAME, SIM3), kind in (FUSE, FUSE_SIM3, BY_SIM3)
    for occ in (0, 1, 2):
        i = b.at(level=1)
        f = b.own(i, occ=occ)
        if not fuse and (occ == 2 or (kf and occ == 1)):
            b.claim(i, "no_candidate", tally=dict(blocked=1))
        else:
            b.claim(i, "matched", f)
    blocking = False
    for flags in (1, 3):
        u, v = b.spot()
        i = b.at(u, v, level=1, flags=flags)
        f = b.own(i)
        j = b.at(u, v, level=1, flags=flags, desc=b.p["desc"][i])
        b.claim(i, "matched", f)
        if not fuse and (kf or flags == 3):
            b.claim(j, "no_candidate", tally=dict(blocked=1))
            b.pair(i, j)
            blocking = True
        else:
            b.claim(j, "matched", f)
    if blocking:
        b.sweeps = 3
    return b.scene()


# ------------------------------------------------------------------ uR and Fuse's gate
def scene_ur_last_frame():
    """mvuRight = -1, 0, the smallest positive floats, and the predicted uR (u - bf/z) a radius away."""
    b = Builder("ur_last_frame", LAST_FRAME)
    tiny, sub = np.finfo(np.float32).tiny, np.nextafter(F32(0), F32(1))
    for ur, ok in ((-1.0, True), (0.0, True), (sub, False), (tiny, False), ("at", True), ("past", False)):
        i = b.at()
        q = b.probe(i)
        if ur in ("at", "past"):  # |ur - uR| == r, and the nearest uR that puts it above r
            past, at, _ = around(float(q["ur"]) - float(q["r"]), lambda x: -abs(F32(q["ur"] - x)), -q["r"])
            ur = at if ur == "at" else past
        f = b.own(i, ur=ur)
        b.claim(i, "matched", f) if ok else b.claim(i, "no_candidate", tally=dict(ur=1))
    b.pair(1, 2)  # mvuRight 0 and the smallest positive float
    b.pair(4, 5)  # |ur - uR| == r and the nearest value above
    return b.scene()


def scene_no_ur(kind, kw):
    """The frame carries no mvuRight at all."""
    b = Builder("no_ur_" + kname(kind, kw.get("frustum")), kind, u_right=False, **kw)
    for level in (0, 1, 2):
        b.matched(b.at(level=level))
    return b.scene()


def _largest_not_above(x):
    t = F32(x)
    return next_down(t) if float(t) > x else t


def scene_fuse_gate():
    """e2 * invSigma2 the largest float not above 5.99 (mono) / 7.8 (stereo) and the next value above; a
    stereo and a mono candidate for one point; mvuRight -1 / 0 / the smallest positive floats (>= 0)."""
    b = Builder("fuse_gate", FUSE)
    for limit, er in ((5.99, None), (7.8, F32(1.0))):
        want = _largest_not_above(limit)
        pair = []
        for _ in range(2):
            i = b.at()
            q = b.probe(i)
            kx = F32(q["x"] - F32(math.sqrt(limit - (1.0 if er else 0.0) - 2e-4)))
            ex = F32(q["x"] - kx)

            def g(ky, q=q, ex=ex):
                ey = F32(q["y"] - ky)
                e2 = F32(F32(ex * ex) + F32(ey * ey))
                if er is not None:
                    e2 = F32(e2 + F32(er * er))
                return F32(e2 * F32(1.0))

            pair.append((i, q, kx, g))
        i, q, kx, g = pair[0]
        _, at, _ = around(float(q["y"]) - 0.0141, lambda ky: -g(ky), -want, 20000)
        f = b.feature(kx, at, 0, b.p["desc"][i], ur=-1.0 if er is None else F32(q["ur"] - er))
        assert er is None or F32(q["ur"] - F32(q["ur"] - er)) == er
        b.claim(i, "matched", f)
        i, q, kx, g = pair[1]
        lo, _, _ = around(float(q["y"]) - 0.0141, lambda ky: -g(ky), -want, 20000)
        assert float(g(lo)) > limit and g(lo) == next_up(want), (g(lo), want)
        b.feature(kx, lo, 0, b.p["desc"][i], ur=-1.0 if er is None else F32(q["ur"] - er))
        b.claim(i, "no_candidate", tally={"gate_mono" if er is None else "gate_stereo": 1})
        b.pair(pair[0][0], pair[1][0])
    i = b.at()
    q = b.probe(i)
    b.feature(q["x"] + F32(2.6), q["y"], 0, b.p["desc"][i])
    f = b.feature(q["x"] - F32(2.6), q["y"], 0, flip_bits(b.p["desc"][i], range(5)), ur=F32(q["ur"] + F32(0.1)))
    b.claim(i, "matched", f, tally=dict(gate_mono=1))
    tiny, sub = np.finfo(np.float32).tiny, np.nextafter(F32(0), F32(1))
    for ur, ok in ((-1.0, True), (0.0, False), (sub, False), (tiny, False)):
        i = b.at()
        f = b.own(i, dx=1.0, ur=ur)
        b.claim(i, "matched", f) if ok else b.claim(i, "no_candidate", tally=dict(gate_stereo=1))
        if ur == 0.0:
            b.pair(i - 1, i)  # mvuRight -1 (mono gate) and 0 (stereo gate)
    return b.scene()


# ------------------------------------------------------------------ Hamming thresholds and ties
def scene_hamming(kind, kw, orb_dist=None):
    """The best distance exactly the threshold and one past it, 0 and 256; ties between two candidates in
    one cell, in two rows of a column, in two columns (the later index in the earlier cell wins) and more
    than 16 enumeration positions apart; 16 and 32 positions apart, which the kernels' 16-lane groups hand to
    one lane (best and runner-up from the same lane), where 1 and 21 apart fall to different lanes."""
    name = "hamming_" + kname(kind, kw.get("frustum")) + ("_%d" % orb_dist if orb_dist else "")
    b = Builder(name, kind, **(dict(kw, orb_dist=orb_dist) if orb_dist else kw))
    thr = orb_dist if orb_dist else THRESHOLD[kind]
    for bits, code in ((thr, "matched"), (thr + 1, "over_threshold"), (0, "matched"), (256, "over_threshold")):
        i = b.at(level=2)
        f = b.own(i, bits=bits)
        b.claim(i, code, f if code == "matched" else None)
    b.pair(0, 1)
    b.pair(2, 3)
    if kind == LOCAL:  # best 41 and second 50 on one level: 41 > 0.8f * 50; adjacent, and in one lane
        for filler in (0, 15):
            i = b.at(level=2)
            f0 = b.own(i, bits=50)
            for m in range(filler):
                b.own(i, dx=0.1 * (m % 5), dy=0.1 * (m // 5), bits=90 + m)
            f1 = b.own(i, dx=0.5, bits=41)
            assert b.apart(i, f0, f1) == filler + 1, b.name
            b.claim(i, "ratio")
    second = 1 if kind == LOCAL else 2  # the local kind: another level, or the ratio test ends the tie
    fr = b.fr
    gx0, gy0 = fr.get("grid_min_x", fr["min_x"]), fr.get("grid_min_y", fr["min_y"])

    def tied(u, v, offs, filler=0):
        i = b.at(u, v, level=2)
        q = b.probe(i)
        d = b.p["desc"][i]
        first = b.feature(q["x"] + F32(offs[0][0]), q["y"] + F32(offs[0][1]), 2, flip_bits(d, range(10)))
        for k in range(filler):
            b.feature(q["x"] + F32(0.1 * (k % 5)), q["y"] + F32(0.1 * (k // 5)), 2, flip_bits(d, range(30, 70 + k)))
        last = b.feature(q["x"] + F32(offs[1][0]), q["y"] + F32(offs[1][1]), second, flip_bits(d, range(10, 20)))
        if filler:
            assert b.apart(i, first, last) == filler + 1, b.name
        return i, first, last

    u, v = b.spot()
    i, first, last = tied(u, v, ((0.0, 0.0), (0.5, 0.0)))
    assert b.apart(i, first, last) == 1, b.name
    b.claim(i, "matched", first)
    u, v = b.spot()
    i, first, last = tied(u, v, ((0.3, 0.2), (0.5, 0.0)), filler=20)
    b.claim(i, "matched", first)
    for filler in (15, 31):  # the same lane of the 16-lane group
        u, v = b.spot()
        i, first, last = tied(u, v, ((0.3, 0.2), (0.5, 0.0)), filler=filler)
        b.claim(i, "matched", first)
    col = float(gx0) + 20.5 / float(fr["grid_inv_w"])  # the edge between grid columns 20 and 21
    i, first, last = tied(col, 300.0, ((2.0, 0.0), (-2.0, 0.0)))
    b.claim(i, "matched", last)
    row = float(gy0) + 30.5 / float(fr["grid_inv_h"])
    i, first, last = tied(420.0, row, ((0.0, 2.0), (0.0, -2.0)))
    b.claim(i, "matched", last)
    g = lit.PyFrame(b.frame()).grid
    where = {f: (cx_, cy_) for cx_ in range(64) for cy_ in range(48) for f in g[cx_][cy_]}
    n = len(b.feats)
    assert where[n - 4][0] == where[n - 3][0] + 1 and where[n - 2] == (where[n - 1][0], where[n - 1][1] + 1), b.name
    return b.scene()


# ------------------------------------------------------------------ the rotation check
def _last_rot_in_bin0():
    """The largest difference whose rot * (1/30.f) still rounds below 0.5 (1/30.f is above 1/30, so the
    float just below 15 already lands on 0.5)."""
    x = F32(15.0)
    while lit._rot_bin(x, 0.0) != 0:
        x = next_down(x)
    return float(x)


ROTATION = {
    # angle differences (count): bins 1 (6), 5 (8) and 8 (7) are the maxima; 14.99.. falls into bin 0,
    # -30 wraps to 330 (bin 11), 900 reaches bin 30, which wraps to 0
    "halves": (((15.0, 1, True), (float(next_up(15.0)), 1, True), (30.0, 4, True), (_last_rot_in_bin0(), 1, False),
                (150.0, 8, True), (240.0, 7, True), (-30.0, 1, False), (900.0, 1, False)), True),
    # first and second maximum tie (the first keeps the lead), the third equals 0.1f * 20 (kept), a fourth
    # ties with the third (not greater: dropped)
    "ties": (((60.0, 20, True), (120.0, 20, True), (180.0, 2, True), (270.0, 2, False)), True),
    "below_tenth": (((60.0, 20, True), (120.0, 1, False), (180.0, 1, False)), True),
    "second_at_tenth": (((60.0, 20, True), (120.0, 2, True), (180.0, 1, False)), True),
    "off": (((15.0, 2, True), (150.0, 8, True), (240.0, 7, True), (-30.0, 1, True), (900.0, 1, True)), False),
}


def scene_rotation(kind, variant):
    groups, check = ROTATION[variant]
    b = Builder("rotation_%s_%s" % (kname(kind), variant), kind, check_ori=check)
    rotates = kind in (LAST_FRAME, KEYFRAME)  # the Sim3 kind keeps no histogram: every match stays
    for diff, count, kept in groups:
        kept = kept or not rotates
        for _ in range(count):
            fa = 40.0 if diff < 0 else 0.0
            i = b.at(angle=fa + diff)
            f = b.own(i, angle=fa)
            b.claim(i, "matched" if kept else "matched_then_rotated_out", f)
    if variant == "halves":
        if rotates:
            b.pair(0, 6)  # differences 15 (bin 1, kept) and the last one of bin 0 (dropped)
        below = F32(_last_rot_in_bin0())
        bins = [lit._rot_bin(F32(d), 0.0) for d in (15.0, next_up(15.0), next_up(below), below, 900.0)]
        assert bins == [1, 1, 1, 0, 0]
        assert lit._rot_bin(F32(900.0), 0.0, "bin30_nowrap") == 30 and lit._rot_bin(F32(10.0), F32(40.0)) == 11
    return b.scene()


# ------------------------------------------------------------------ the Sim3 decomposition on a general pose
def scene_sim3_pose(kind, s):
    """Scw = s [R | t] with a general rotation: the squared norm of row 0 is not exact in float."""
    b = Builder("sim3_pose_%s_s%g" % (kname(kind), s), kind)
    ax = np.array([0.3, 0.5, 0.2])
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(0.07) * K + (1 - math.cos(0.07)) * K @ K
    S = np.eye(4)
    S[:3, :3], S[:3, 3] = s * R, s * np.array([0.1, -0.2, 0.3])
    b.fr["Tcw"] = S.astype(np.float32)
    row = b.fr["Tcw"][0, :3].astype(np.float64)
    assert float(F32(row @ row)) != float(row @ row)
    for k in range(12):
        b.matched(b.at(z=3.0 + k, level=k % 4), bits=k)
    return b.scene()


# ------------------------------------------------------------------ sweeps
def scene_chain(kind, d, flags=3, kw=None):
    """d identical points over d co-located features at distances 0 .. d-1: every sweep frees one more
    point from the feature its predecessors took, d + 1 sweeps in all (the count is checked with
    py_sweeps, not assumed).  flags=1 (no observations) under the local / last-frame kinds: nothing blocks."""
    kw = kw or {}
    b = Builder("chain_%s_%d%s" % (kname(kind, kw.get("frustum")), d, "" if flags == 3 else "_unflagged"), kind, **kw)
    u, v = b.spot()
    first = b.at(u, v, level=2, flags=flags)
    feats = [b.own(first, bits=k, octave=2 - (k & 1)) for k in range(d)]  # alternate levels: no ratio test
    b.claim(first, "matched", feats[0])
    blocks = kind in (KEYFRAME, SIM3) or (kind in (LOCAL, LAST_FRAME) and flags == 3)
    for k in range(1, d):
        j = b.at(u, v, level=2, flags=flags, desc=b.p["desc"][first])
        b.claim(j, "matched", feats[k] if blocks else feats[0])
    fuse = kind in (FUSE, FUSE_SIM3, BY_SIM3)
    b.sweeps = 1 if fuse else (d + 1 if blocks else 2)
    return b.scene()


def scene_no_points(kind):
    b = Builder("no_points_" + kname(kind), kind)
    i = b.at()
    b.own(i)
    for key in b.p:
        b.p[key].pop()
    b.sweeps = 1
    return b.scene()


# ------------------------------------------------------------------ shapes
def scene_shape(kind, kw, nF, nP):
    """nF random features (the bitonic sort pads to a power of two), nP points each aimed at one of them."""
    b = Builder("shape_%s_f%d_p%d" % (kname(kind, kw.get("frustum")), nF, nP), kind, **kw)
    g = b.g
    for _ in range(nF):
        b.feature(g.uniform(10, W - 10), g.uniform(10, H - 10), int(g.integers(0, 3)), b.desc(),
                  ur=-1.0 if g.random() < 0.5 else float(g.uniform(1, 600)), occ=int(g.integers(0, 3)),
                  angle=float(g.uniform(0, 360)))
    for i in range(nP):
        f = int(g.integers(0, nF))
        x, y, o, a = b.feats[f]
        b.at(float(x) + float(g.normal(0, 0.5)), float(y) + float(g.normal(0, 0.5)), z=float(g.uniform(2, 20)),
             level=min(o + int(g.integers(0, 2)), 7), desc=flip_bits(b.fdesc[f], range(int(g.integers(0, 30)))),
             flags=int(g.integers(0, 4)), angle=float(a))
    b.sweeps = -1  # whatever the model reports
    return b.scene()


# ------------------------------------------------------------------ the table
# every scene of the table, written out so that collecting the tests builds none of them
SCENE_NAMES = (
    "occupancy_local", "no_ur_local", "hamming_local", "depth_last_frame", "bounds_last_frame",
    "occupancy_last_frame", "no_ur_last_frame", "hamming_last_frame", "depth_keyframe", "bounds_keyframe",
    "distance_keyframe", "predict_keyframe_s1.2_n8", "occupancy_keyframe", "no_ur_keyframe", "depth_fuse",
    "bounds_fuse", "distance_fuse", "predict_fuse_s1.2_n8", "occupancy_fuse", "no_ur_fuse", "hamming_fuse",
    "depth_sim3", "bounds_sim3", "distance_sim3", "predict_sim3_s1.2_n8", "occupancy_sim3", "no_ur_sim3",
    "hamming_sim3", "depth_fuse_sim3", "bounds_fuse_sim3", "distance_fuse_sim3", "predict_fuse_sim3_s1.2_n8",
    "occupancy_fuse_sim3", "no_ur_fuse_sim3", "hamming_fuse_sim3", "depth_by_sim3", "bounds_by_sim3",
    "distance_by_sim3", "predict_by_sim3_s1.2_n8", "occupancy_by_sim3", "no_ur_by_sim3", "hamming_by_sim3",
    "depth_local_frustum", "bounds_local_frustum", "distance_local_frustum", "predict_local_frustum_s1.2_n8",
    "occupancy_local_frustum", "no_ur_local_frustum", "hamming_local_frustum", "predict_keyframe_s1.5_n4",
    "predict_local_frustum_s1.5_n4", "predict_keyframe_s1.1_n12", "predict_local_frustum_s1.1_n12",
    "predict_keyframe_s1.2_n1", "predict_local_frustum_s1.2_n1", "predict_keyframe_s1.1_n16",
    "predict_local_frustum_s1.1_n16", "local_th1", "local_th3", "out_of_pyramid_local", "out_of_pyramid_last_frame",
    "last_frame_levels_at_b", "last_frame_levels_above_b", "last_frame_levels_below_b",
    "last_frame_levels_at_minus_b", "last_frame_levels_below_minus_b", "last_frame_levels_above_minus_b",
    "last_frame_levels_mono_far", "ur_last_frame", "fuse_gate", "hamming_keyframe_100", "hamming_keyframe_64",
    "hamming_keyframe_50", "rotation_last_frame_halves", "rotation_last_frame_ties",
    "rotation_last_frame_below_tenth", "rotation_last_frame_second_at_tenth", "rotation_last_frame_off",
    "rotation_keyframe_halves", "rotation_keyframe_ties", "rotation_keyframe_below_tenth",
    "rotation_keyframe_second_at_tenth", "rotation_keyframe_off", "rotation_sim3_halves", "local_cell_edges",
    "sim3_pose_sim3_s1", "sim3_pose_sim3_s0.35", "sim3_pose_sim3_s2.9", "sim3_pose_fuse_sim3_s1",
    "sim3_pose_fuse_sim3_s0.35", "sim3_pose_fuse_sim3_s2.9", "chain_keyframe_1", "chain_keyframe_2",
    "chain_keyframe_3", "chain_keyframe_4", "chain_keyframe_5", "chain_keyframe_40", "chain_last_frame_1",
    "chain_last_frame_2", "chain_last_frame_3", "chain_last_frame_4", "chain_last_frame_5", "chain_last_frame_40",
    "chain_local_2", "chain_local_3", "chain_local_4", "chain_sim3_3", "chain_sim3_4",
    "chain_last_frame_4_unflagged", "chain_fuse_4", "chain_by_sim3_3", "no_points_keyframe", "no_points_fuse",
    "no_points_last_frame", "shape_keyframe_f1_p1", "shape_last_frame_f2_p63", "shape_fuse_f3_p64",
    "shape_local_frustum_f1023_p65", "shape_sim3_f1024_p1", "shape_local_f1025_p64", "shape_fuse_sim3_f3_p65",
    "shape_by_sim3_f1024_p63", "shape_keyframe_f1025_p65", "shape_keyframe_f3_p4100",
)
HOST_SCENE_NAMES = tuple(n for n in SCENE_NAMES if not n.startswith("out_of_pyramid_"))  # the host call refuses those
SHAPES = ((1, 1), (2, 63), (3, 64), (1023, 65), (1024, 1), (1025, 64), (3, 65), (1024, 63))


def _table():
    """One builder per scene, in the order of SCENE_NAMES; nothing is built here."""
    P = functools.partial
    out = []
    for kind, kw in variants():
        given = kind == LOCAL and not kw  # the local kind without the frustum takes given track fields
        if not given:
            out += [P(scene_depth, kind, kw), P(scene_bounds, kind, kw)]
        if not given and kind != LAST_FRAME:
            out += [P(scene_distance, kind, kw), P(scene_predict, kind, kw)]
        out += [P(scene_occupancy, kind, kw), P(scene_no_ur, kind, kw)]
        if kind != KEYFRAME:
            out.append(P(scene_hamming, kind, kw))
    for scale, nlevels in PYRAMIDS[1:]:
        out += [P(scene_predict, KEYFRAME, {}, scale, nlevels),
                P(scene_predict, LOCAL, dict(frustum=True), scale, nlevels)]
    out += [P(scene_local, 1.0), P(scene_local, 3.0), P(scene_out_of_pyramid, LOCAL),
            P(scene_out_of_pyramid, LAST_FRAME)]
    out += [P(scene_last_frame_levels, m) for m in LAST_FRAME_MODES]
    out += [scene_ur_last_frame, scene_fuse_gate]
    out += [P(scene_hamming, KEYFRAME, {}, d) for d in (100, 64, 50)]
    out += [P(scene_rotation, k, v) for k in (LAST_FRAME, KEYFRAME) for v in ROTATION]
    out += [P(scene_rotation, SIM3, "halves"), scene_cell_edges]
    out += [P(scene_sim3_pose, k, s) for k in (SIM3, FUSE_SIM3) for s in (1.0, 0.35, 2.9)]
    for kind in (KEYFRAME, LAST_FRAME):
        out += [P(scene_chain, kind, d) for d in (1, 2, 3, 4, 5, 40)]
    out += [P(scene_chain, LOCAL, d) for d in (2, 3, 4)] + [P(scene_chain, SIM3, d) for d in (3, 4)]
    out += [P(scene_chain, LAST_FRAME, 4, flags=1), P(scene_chain, FUSE, 4), P(scene_chain, BY_SIM3, 3)]
    out += [P(scene_no_points, KEYFRAME), P(scene_no_points, FUSE), P(scene_no_points, LAST_FRAME)]
    kinds = ((KEYFRAME, {}), (LAST_FRAME, {}), (FUSE, {}), (LOCAL, dict(frustum=True)), (SIM3, {}), (LOCAL, {}),
             (FUSE_SIM3, {}), (BY_SIM3, {}))
    out += [P(scene_shape, k, kw, nF, nP) for (k, kw), (nF, nP) in zip(kinds, SHAPES)]
    out.append(P(scene_shape, KEYFRAME, {}, 1025, 65))  # the device-sized batch truncates this one
    out.append(P(scene_shape, KEYFRAME, {}, 3, 4100))   # the 64 split blocks loop over their points
    assert len(out) == len(SCENE_NAMES) == len(set(SCENE_NAMES))
    return out


@functools.lru_cache(maxsize=None)
def by_name(name):
    """The scene of that name, built on first use (tests are parametrised over the static SCENE_NAMES, so
    collecting them builds nothing)."""
    s = _table()[SCENE_NAMES.index(name)]()
    assert s["name"] == name, (s["name"], name)
    assert s["host"] == (name in HOST_SCENE_NAMES), name
    return s


def all_scenes():
    return tuple(by_name(n) for n in SCENE_NAMES)


def call_kw(s):
    """The scene's arguments in py_search's spelling."""
    kw = dict(s["kw"])
    kw["limit"] = kw.pop("view_cos_limit", 0.5)
    return kw


@functools.lru_cache(maxsize=None)
def literal_result(name):
    s = by_name(name)
    return lit.py_search(s["fr"], s["pts"], s["kind"], **call_kw(s))


def sim3_pair(s):
    """A BY_SIM3 scene as the first direction of a whole SearchBySim3 call with s12 = 1, R12 = I, t12 = 0:
    KF1 gets one feature per point on a lattice of its own, and every KF2 feature that the first direction
    reaches gets a MapPoint that projects back onto the KF1 feature of the first point matched to it, so
    the mutual check keeps that match.  Returns (kf1, kf2, pts1, pts2, s12, R12, t12, th)."""
    assert s["kind"] == BY_SIM3 and np.array_equal(s["kw"]["last_Tcw"], np.eye(4, dtype=np.float32))
    n1, n2 = len(s["pts"]["desc"]), len(s["fr"]["desc"])
    assert n1 <= 30 * 22
    b1 = Builder("kf1", BY_SIM3, seed=77)
    for i in range(n1):
        b1.feature(30.0 + 20.0 * (i % 30), 30.0 + 20.0 * (i // 30), 0, b1.desc())
    kf1 = b1.frame()
    kf1["Tcw"] = np.asarray(s["fr"]["Tcw"], np.float32)
    kf2 = dict(s["fr"], Tcw=np.eye(4, dtype=np.float32))
    m1 = literal_result(s["name"])["point_match"]
    b2 = Builder("kf2", BY_SIM3)  # its points project into KF1 through the identity
    for f in range(n2):
        first = [i for i in range(n1) if m1[i] == f]
        if first:
            x, y, _, _ = b1.feats[first[0]]
            b2.at(float(x), float(y), level=0, desc=b1.fdesc[first[0]], flags=1)
        else:
            b2.raw_point(flags=0)
    return (kf1, kf2, s["pts"], b2.points(), F32(1.0), np.eye(3, dtype=np.float32), np.zeros(3, np.float32),
            s["kw"]["th"])

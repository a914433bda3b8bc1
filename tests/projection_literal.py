"""A literal pure-Python restatement of the SearchByProjection family (src/ORBmatcher.cc:46-151, 327-440,
944-1236, 1238-1487, 1489-1839, src/Frame.cc:254-453, src/MapPoint.cc:407-440), one statement per
statement of the reference, with every float operation rounded where the reference rounds it.

Beyond the results (nmatches, frame_out, point_match[, track, track_level]) it reports, per point, HOW
the point's turn ended (`exit`, one of EXITS) and how many candidates each filter removed (`tally`, keys
TALLIES), so that a crafted scene (tests/projection_scenes.py) can claim the exit and the filter it is
built for.  `defect=` switches in one-token mutations (DEFECTS) to show that the scenes tell them apart.

py_sweeps() is the kernels' Jacobi iteration written plainly over the same per-point search: every
point against the previous sweep's first-writer table until nothing changes.  It returns the sequential
scan's result plus the number of sweeps, which is what a scene states to sit on either side of the
split kernels' hand-over.

Choices the source does not determine, stated here as the oracle and the kernels do:
  * u != u || v != v ends the point (0 * inf) where the bounds test is `u < min || u > max`; the
    IsInImage form `!(u >= min && u < max ...)` rejects a NaN by itself, so those kinds report
    out_of_image and never nan_uv;
  * PredictScale of a NaN quotient is level 0, of +-inf the top / bottom level;
  * a local point with a track level outside the pyramid, and a last-frame point with an octave outside
    it, end their turn (level_unset, octave_range): the reference would index out of its tables.
"""
import math

import numpy as np

import oracle

f32 = np.float32

LOCAL, LAST_FRAME, KEYFRAME, FUSE, SIM3, FUSE_SIM3, BY_SIM3 = range(7)
KIND_NAMES = ("local", "last_frame", "keyframe", "fuse", "sim3", "fuse_sim3", "by_sim3")

EXITS = ("flag_off", "level_unset", "behind", "nan_uv", "out_of_image", "distance", "view_cos", "normal",
         "octave_range", "no_candidate", "over_threshold", "ratio", "matched", "matched_then_rotated_out")
TALLIES = ("level", "radius", "blocked", "ur", "gate_stereo", "gate_mono")

# one-token mutations (test_scenes_reject_seeded_defects)
DEFECTS = ("radius_le",            # |dx| < r  ->  <=
           "ur_ge",                # searches: mvuRight > 0  ->  >= 0
           "fuse_ur_gt",           # Fuse's gate: mvuRight >= 0  ->  > 0
           "bounds_le",            # IsInImage: u < max_x  ->  <=
           "viewcos_ge",           # RadiusByViewingCos: > 0.998  ->  >=
           "ratio_any_level",      # the ratio test also when best and second differ in level
           "second_level_last",    # bestLevel2 only from the `dist < bestDist2` branch
           "tie_later",            # dist < bestDist  ->  <=
           "predict_floor",        # PredictScale: ceil -> floor
           "bin30_nowrap",         # rotation bin 30 kept
           "maxima_le",            # ComputeThreeMaxima: max2 < 0.1f*max1  ->  <=
           "unflagged_blocks",     # a match by a point without observations blocks later points
           "occ1_blocks_local",    # an occupant without observations blocks the local / last-frame kinds
           "invz_float")           # Fuse(KeyFrame*, Scw): invz = 1.0/z formed in float

_FUSE_FAMILY = (FUSE, FUSE_SIM3, BY_SIM3)   # no "already matched" state
_KF_FAMILY = (KEYFRAME, SIM3)               # any MapPoint on a feature blocks it, every match blocks
_ROTATING = (LAST_FRAME, KEYFRAME)
_ORDER = {LOCAL: ("level", "radius", "blocked", "ur"), LAST_FRAME: ("level", "radius", "blocked", "ur"),
          KEYFRAME: ("level", "radius", "blocked"), FUSE: ("radius", "level", "gate"),
          SIM3: ("radius", "blocked", "level"), FUSE_SIM3: ("radius", "level"), BY_SIM3: ("radius", "level")}
_INF = 1 << 30


def _mat3x1(T, X):
    """R*X + t: OpenCV 3.2 cv::gemm small-matrix path -- float dot product left to right, then a
    correctly rounded float add of t."""
    out = []
    for r in range(3):
        t0 = f32(f32(f32(T[r, 0]) * f32(X[0])) + f32(f32(T[r, 1]) * f32(X[1])))
        t0 = f32(t0 + f32(f32(T[r, 2]) * f32(X[2])))
        out.append(f32(float(t0) + float(T[r, 3])))
    return out


def _centre(T):
    return [f32(-((float(T[0, c]) * float(T[0, 3]) + float(T[1, c]) * float(T[1, 3])) + float(T[2, c]) * float(T[2, 3])))
            for c in range(3)]


def _centre_kf(T):
    """KeyFrame::GetCameraCenter: Ow = -Rwc*tcw with Rwc a Mat (src/KeyFrame.cc:84-87): cv::gemm's
    small-matrix path, the dot product in float, alpha = -1."""
    out = []
    for c in range(3):
        t0 = f32(f32(f32(T[0, c]) * f32(T[0, 3])) + f32(f32(T[1, c]) * f32(T[1, 3])))
        out.append(-f32(t0 + f32(f32(T[2, c]) * f32(T[2, 3]))))
    return out


def _norm3(v):
    s = float(v[0]) * float(v[0])
    s = s + float(v[1]) * float(v[1])
    s = s + float(v[2]) * float(v[2])
    return f32(math.sqrt(s))


def _dot3(a, b):
    s = float(a[0]) * float(b[0])
    s = s + float(a[1]) * float(b[1])
    s = s + float(a[2]) * float(b[2])
    return s


def _inv_float(z):
    """1.0f / z"""
    with np.errstate(divide="ignore"):
        return f32(f32(1.0) / f32(z))


def _inv_double(z):
    """(float)(1.0 / (double)z)"""
    with np.errstate(divide="ignore"):
        return f32(np.float64(1.0) / np.float64(z))


def _mul(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return f32(f32(a) * f32(b))


def _add(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return f32(f32(a) + f32(b))


def predict_quotient(dmax, dist, logsf):
    """The float PredictScale takes the ceiling of: log(dmax / dist) / log(scaleFactor)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = f32(f32(dmax) / f32(dist))
        return f32(f32(oracle.log_det(ratio)) / f32(logsf))


def _predict(dmax, dist, logsf, nl, defect=None):
    q = predict_quotient(dmax, dist, logsf)
    if q != q:
        n = 0
    elif q > f32(1e6):
        n = nl - 1
    elif q < f32(-1e6):
        n = 0
    else:
        n = int(math.floor(q)) if defect == "predict_floor" else int(math.ceil(q))
    return min(max(n, 0), nl - 1)


def sim3_decompose(S):
    """Scw -> [Rcw | tcw] = [sRcw | t] / scw (src/ORBmatcher.cc:335-339): Mat / scw is convertTo(alpha =
    1/scw), a float scale."""
    S = np.asarray(S, np.float32)
    d = float(S[0, 0]) * float(S[0, 0])
    d = d + float(S[0, 1]) * float(S[0, 1])
    d = d + float(S[0, 2]) * float(S[0, 2])
    a = f32(1.0 / float(f32(math.sqrt(d))))
    T = np.eye(4, dtype=np.float32)
    T[:3, :] = (S[:3, :] * a).astype(np.float32) + f32(0.0)  # x * alpha + 0.0f
    return T


class PyFrame:
    """Frame::AssignFeaturesToGrid / GetFeaturesInArea, src/Frame.cc:254-271, 388-453."""

    def __init__(self, fr):
        self.fr = fr
        k = fr["keys_un"]
        self.grid = [[[] for _ in range(48)] for _ in range(64)]
        for i in range(len(k)):
            # PosInGrid's round() is half-away-from-zero
            # a KeyFrame's grid is its Frame's, built with the float bounds (grid_min_*); its
            # GetFeaturesInArea below uses the KeyFrame's integer copies (min_x / min_y)
            gx0, gy0 = fr.get("grid_min_x", fr["min_x"]), fr.get("grid_min_y", fr["min_y"])
            vx = float(f32(f32(k["x"][i] - f32(gx0)) * fr["grid_inv_w"]))
            vy = float(f32(f32(k["y"][i] - f32(gy0)) * fr["grid_inv_h"]))
            px = int(math.floor(abs(vx) + 0.5)) * (1 if vx >= 0 else -1)
            py = int(math.floor(abs(vy) + 0.5)) * (1 if vy >= 0 else -1)
            if 0 <= px < 64 and 0 <= py < 48:
                self.grid[px][py].append(i)

    def cell_range(self, x, y, r):
        """(x0, x1, y0, y1) of GetFeaturesInArea, or None where it returns empty-handed."""
        fr = self.fr
        x, y, r = f32(x), f32(y), f32(r)
        x0 = max(0, int(math.floor(f32(f32(f32(x - fr["min_x"]) - r) * fr["grid_inv_w"]))))
        if x0 >= 64:
            return None
        x1 = min(63, int(math.ceil(f32(f32(f32(x - fr["min_x"]) + r) * fr["grid_inv_w"]))))
        if x1 < 0:
            return None
        y0 = max(0, int(math.floor(f32(f32(f32(y - fr["min_y"]) - r) * fr["grid_inv_h"]))))
        if y0 >= 48:
            return None
        y1 = min(47, int(math.ceil(f32(f32(f32(y - fr["min_y"]) + r) * fr["grid_inv_h"]))))
        if y1 < 0:
            return None
        return x0, x1, y0, y1

    def cells(self, x, y, r):
        """Every feature of the window's cells in the reference's enumeration order (cell x, cell y, index)."""
        cr = self.cell_range(x, y, r)
        if cr is None:
            return []
        x0, x1, y0, y1 = cr
        return [j for ix in range(x0, x1 + 1) for iy in range(y0, y1 + 1) for j in self.grid[ix][iy]]

    @staticmethod
    def level_rejects(octave, minL, maxL):
        check = minL > 0 or maxL >= 0
        return bool(check and (octave < minL or (maxL >= 0 and octave > maxL)))

    def area(self, x, y, r, minL=-1, maxL=-1):
        k = self.fr["keys_un"]
        x, y, r = f32(x), f32(y), f32(r)
        out = []
        for j in self.cells(x, y, r):
            if self.level_rejects(k["octave"][j], minL, maxL):
                continue
            if abs(f32(k["x"][j] - x)) < r and abs(f32(k["y"][j] - y)) < r:
                out.append(j)
        return out


def _ham(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def _rot_bin(a, b, defect=None):
    rot = f32(f32(a) - f32(b))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    v = float(f32(rot * f32(1.0 / 30)))
    b_ = int(math.floor(v + 0.5))
    return 0 if b_ == 30 and defect != "bin30_nowrap" else b_


def _three_max(counts, defect=None):
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(counts):
        if s > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif s > m2:
            m3, m2, i3, i2 = m2, s, i2, i
        elif s > m3:
            m3, i3 = s, i
    lim = f32(0.1) * f32(m1)
    below = (lambda m: m <= lim) if defect == "maxima_le" else (lambda m: m < lim)
    if below(m2):
        i2 = i3 = -1
    elif below(m3):
        i3 = -1
    return i1, i2, i3


class Search:
    """One problem: everything the reference derives before its point loop, and the per-point search
    (`point`) that the sequential scan (py_search) and the sweep model (py_sweeps) both call."""

    def __init__(self, fr, pts, kind, th, nnratio=0.6, check_ori=True, mono=False, orb_dist=100, last_Tcw=None,
                 frustum=False, limit=0.5, defect=None):
        assert defect is None or defect in DEFECTS, defect
        self.fr, self.pts, self.kind, self.th, self.defect = fr, pts, kind, th, defect
        self.nnratio, self.check_ori, self.mono, self.orb_dist = nnratio, check_ori, mono, orb_dist
        self.frustum, self.limit = bool(frustum) and kind == LOCAL, limit
        self.F = PyFrame(fr)
        self.keys, self.n = fr["keys_un"], len(fr["keys_un"])
        self.npnt = len(pts["desc"])
        self.occ, self.ur = fr.get("occ"), fr.get("u_right")
        T = np.asarray(fr["Tcw"], np.float32)
        if kind in (SIM3, FUSE_SIM3):
            T = sim3_decompose(T)
        self.T = T
        self.Ow = _centre_kf(T) if kind == FUSE else _centre(T)  # Fuse: pKF->GetCameraCenter()
        self.A = None if last_Tcw is None else np.asarray(last_Tcw, np.float32)
        self.fwd = self.bwd = False
        if kind == LAST_FRAME:
            self.tlc = _mat3x1(self.A, self.Ow)
            self.fwd = bool(self.tlc[2] > fr["b"] and not mono)
            self.bwd = bool(-self.tlc[2] > fr["b"] and not mono)
        self.cam = tuple(f32(fr[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
        self.sf = fr["scale_factors"]
        isg = fr.get("inv_level_sigma2")
        self.isg = [f32(isg[l]) if isg is not None else f32(f32(1.0) / f32(self.sf[l] * self.sf[l]))
                    for l in range(int(fr["nlevels"]))]
        given = kind == LOCAL and not self.frustum
        self.track = np.array(pts["track"], np.float32) if given else np.zeros((self.npnt, 4), np.float32)
        self.level = np.array(pts["track_level"], np.int32) if given else np.full(self.npnt, -1, np.int32)
        self.frustum_exit = [None] * self.npnt
        if self.frustum:
            for i in range(self.npnt):
                self.frustum_exit[i] = self._in_frustum(i)

    # ---- Frame::isInFrustum, src/Frame.cc:315-375
    def _in_frustum(self, i):
        fr, pts = self.fr, self.pts
        fx, fy, cx, cy, bf = self.cam
        if not (pts["flags"][i] & 1):
            return "flag_off"
        P = pts["pos"][i]
        code, u, v, invz, _ = self.uv(i)
        if code:
            return code
        if u < fr["min_x"] or u > fr["max_x"] or v < fr["min_y"] or v > fr["max_y"]:
            return "out_of_image"
        PO = [f32(P[j] - self.Ow[j]) for j in range(3)]
        d = _norm3(PO)
        dmin, dmax = pts["dist_minmax"][i]
        if d < f32(f32(0.8) * dmin) or d > f32(f32(1.2) * dmax):
            return "distance"
        with np.errstate(divide="ignore", invalid="ignore"):
            vc = f32(np.float64(_dot3(PO, pts["normal"][i])) / np.float64(d))
        if vc < f32(self.limit):
            return "view_cos"
        self.level[i] = _predict(dmax, d, fr["log_scale_factor"], fr["nlevels"], self.defect)
        self.track[i] = [u, v, f32(u - _mul(bf, invz)), vc]
        return None

    # ---- the projection as each kind forms it, before its bounds test
    def uv(self, i):
        """(exit code or None, u, v, invz, camera coordinates) of point i."""
        fx, fy, cx, cy, _ = self.cam
        kind = self.kind
        X = self.pts["pos"][i]
        if kind == BY_SIM3:  # one direction of SearchBySim3, :1283-1340
            c = _mat3x1(self.A, _mat3x1(self.T, X))
        else:
            c = _mat3x1(self.T, X)
        if kind in (FUSE, SIM3, FUSE_SIM3, BY_SIM3):
            if c[2] < 0:
                return "behind", None, None, None, c
            double = kind in (FUSE_SIM3, BY_SIM3) and self.defect != "invz_float"
            invz = _inv_double(c[2]) if double else _inv_float(c[2])
            u = _add(_mul(fx, _mul(c[0], invz)), cx)
            v = _add(_mul(fy, _mul(c[1], invz)), cy)
            return None, u, v, invz, c
        if kind == LOCAL:  # isInFrustum
            if c[2] < 0:
                return "behind", None, None, None, c
            invz = _inv_float(c[2])
        else:
            invz = _inv_double(c[2])
            if kind == LAST_FRAME and invz < 0:
                return "behind", None, None, None, c
        u = _add(_mul(_mul(fx, c[0]), invz), cx)
        v = _add(_mul(_mul(fy, c[1]), invz), cy)
        if u != u or v != v:  # 0 * inf: undefined in the reference
            return "nan_uv", None, None, None, c
        return None, u, v, invz, c

    # ---- everything before the candidate loop: an exit code, or the query
    def query(self, i):
        fr, pts, kind = self.fr, self.pts, self.kind
        fx, fy, cx, cy, bf = self.cam
        nl = int(fr["nlevels"])
        fl = pts["flags"][i]
        if kind == LOCAL:
            if self.frustum:
                if self.frustum_exit[i] is not None:
                    return self.frustum_exit[i]
            elif not (fl & 1):
                return "flag_off"
            lv = int(self.level[i])
            if lv < 0 or lv >= nl:
                return "level_unset"
            tr = self.track[i]
            wide = tr[3] >= f32(0.998) if self.defect == "viewcos_ge" else tr[3] > f32(0.998)
            r = f32(2.5) if wide else f32(4.0)  # RadiusByViewingCos
            if f32(self.th) != f32(1.0):
                r = f32(r * f32(self.th))
            rs = f32(r * self.sf[lv])
            return dict(x=tr[0], y=tr[1], r=rs, minL=lv - 1, maxL=lv, ur=tr[2], thr=100, level=lv)
        if not (fl & 1):
            return "flag_off"
        X = pts["pos"][i]
        code, u, v, invz, c = self.uv(i)
        if code:
            return code
        if kind in (FUSE, SIM3, FUSE_SIM3, BY_SIM3):
            if self.defect == "bounds_le":
                inside = u >= fr["min_x"] and u <= fr["max_x"] and v >= fr["min_y"] and v <= fr["max_y"]
            else:
                inside = u >= fr["min_x"] and u < fr["max_x"] and v >= fr["min_y"] and v < fr["max_y"]
            if not inside:  # KeyFrame::IsInImage: false for a NaN too
                return "out_of_image"
            assert u == u and v == v  # nan_uv cannot be reached by these kinds
            PO = c if kind == BY_SIM3 else [f32(X[j] - self.Ow[j]) for j in range(3)]
            d3 = _norm3(PO)
            dmin, dmax = pts["dist_minmax"][i]
            if d3 < f32(f32(0.8) * dmin) or d3 > f32(f32(1.2) * dmax):
                return "distance"
            if kind != BY_SIM3 and _dot3(PO, pts["normal"][i]) < 0.5 * float(d3):
                return "normal"
            lv = _predict(dmax, d3, fr["log_scale_factor"], nl, self.defect)
            rad = f32(f32(self.th) * self.sf[lv])
            return dict(x=u, y=v, r=rad, minL=lv - 1, maxL=lv, ur=f32(u - _mul(bf, invz)),
                        thr=100 if kind == BY_SIM3 else 50, level=lv)
        invzc = invz
        if u < fr["min_x"] or u > fr["max_x"] or v < fr["min_y"] or v > fr["max_y"]:
            return "out_of_image"
        if kind == LAST_FRAME:
            o = int(pts["octave"][i])
            if o < 0 or o >= nl:
                return "octave_range"
            rad = f32(f32(self.th) * self.sf[o])
            if self.fwd:
                minL, maxL = o, -1
            elif self.bwd:
                minL, maxL = 0, o
            else:
                minL, maxL = o - 1, o + 1
            return dict(x=u, y=v, r=rad, minL=minL, maxL=maxL, ur=f32(u - _mul(bf, invzc)), thr=100, level=o)
        PO = [f32(X[j] - self.Ow[j]) for j in range(3)]
        d3 = _norm3(PO)
        dmin, dmax = pts["dist_minmax"][i]
        if d3 < f32(f32(0.8) * dmin) or d3 > f32(f32(1.2) * dmax):
            return "distance"
        lv = _predict(dmax, d3, fr["log_scale_factor"], nl, self.defect)
        rad = f32(f32(self.th) * self.sf[lv])
        return dict(x=u, y=v, r=rad, minL=lv - 1, maxL=lv + 1, ur=None, thr=self.orb_dist, level=lv)

    def d3(self, i):
        """The distance the bounds test and PredictScale take (crafting aid; query() forms it the same way)."""
        X = self.pts["pos"][i]
        if self.kind == BY_SIM3:
            return _norm3(_mat3x1(self.A, _mat3x1(self.T, X)))
        return _norm3([f32(X[j] - self.Ow[j]) for j in range(3)])

    def gate_value(self, q, idx):
        """Fuse's reprojection gate for candidate idx: (e2 * invSigma2 as float, stereo?)."""
        keys, ur = self.keys, self.ur
        kl = int(keys["octave"][idx])
        ex, ey = f32(q["x"] - keys["x"][idx]), f32(q["y"] - keys["y"][idx])
        stereo = ur is not None and (ur[idx] > 0 if self.defect == "fuse_ur_gt" else ur[idx] >= 0)
        if stereo:
            er = f32(q["ur"] - ur[idx])
            e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))
        else:
            e2 = f32(f32(ex * ex) + f32(ey * ey))
        return f32(e2 * self.isg[kl]), bool(stereo)

    # ---- one point's turn: (match, exit code before the rotation check, tallies)
    def point(self, i, blocked):
        """blocked(idx): the feature is hidden from point i (occupied on entry, or matched by an earlier
        blocking point)."""
        tally = dict.fromkeys(TALLIES, 0)
        q = self.query(i)
        if isinstance(q, str):
            return -1, q, tally
        kind, keys, ur, defect = self.kind, self.keys, self.ur, self.defect
        x, y, r = f32(q["x"]), f32(q["y"]), f32(q["r"])
        dq = self.pts["desc"][i]
        bd, bl, bd2, bl2, bi = 256, -1, 256, -1, -1
        seen = 0
        for idx in self.F.cells(x, y, r):
            removed = None
            for f in _ORDER[kind]:
                if f == "level":
                    if PyFrame.level_rejects(int(keys["octave"][idx]), q["minL"], q["maxL"]):
                        removed = "level"
                elif f == "radius":
                    dx, dy = abs(f32(keys["x"][idx] - x)), abs(f32(keys["y"][idx] - y))
                    if not ((dx <= r and dy <= r) if defect == "radius_le" else (dx < r and dy < r)):
                        removed = "radius"
                elif f == "blocked":
                    if blocked(idx):
                        removed = "blocked"
                elif f == "ur":
                    if ur is not None and (ur[idx] >= 0 if defect == "ur_ge" else ur[idx] > 0):
                        if abs(f32(q["ur"] - ur[idx])) > r:
                            removed = "ur"
                elif f == "gate":
                    g, stereo = self.gate_value(q, idx)
                    if float(g) > (7.8 if stereo else 5.99):
                        removed = "gate_stereo" if stereo else "gate_mono"
                if removed:
                    break
            if removed:
                tally[removed] += 1
                continue
            seen += 1
            d = _ham(dq, self.fr["desc"][idx])
            lvl = int(keys["octave"][idx])
            if (d <= bd) if defect == "tie_later" else (d < bd):
                if defect != "second_level_last":
                    bl2 = bl
                bd2, bd, bl, bi = bd, d, lvl, idx
            elif d < bd2:
                bl2, bd2 = lvl, d
        if seen == 0:
            return -1, "no_candidate", tally
        if bd > q["thr"]:
            return -1, "over_threshold", tally
        if kind == LOCAL and (bl == bl2 or defect == "ratio_any_level") and \
                f32(bd) > f32(f32(self.nnratio) * f32(bd2)):
            return -1, "ratio", tally
        return bi, "matched", tally

    def blocks(self, i):
        """A match by point i hides its feature from later points."""
        if self.kind in _FUSE_FAMILY:
            return False
        if self.kind in _KF_FAMILY:
            return True
        return bool(self.pts["flags"][i] & 2) or self.defect == "unflagged_blocks"

    def occupied(self, idx):
        """The feature is hidden from every point by what it held on entry."""
        o = 0 if self.occ is None else int(self.occ[idx])
        if self.kind in _FUSE_FAMILY:
            return False
        if self.kind in _KF_FAMILY:
            return o != 0
        return o == 2 or (o == 1 and self.defect == "occ1_blocks_local")

    # ---- after the point loop: the rotation check, frame_out, the count
    def finish(self, pm, exits, tallies, who):
        kind = self.kind
        nm = sum(1 for m in pm if m >= 0)
        if kind in _ROTATING and self.check_ori:
            hist = [[] for _ in range(31)]
            for i, m in enumerate(pm):
                if m >= 0:
                    hist[_rot_bin(self.pts["angle"][i], self.keys["angle"][m], self.defect)].append((i, m))
            sel = _three_max([len(h) for h in hist[:30]], self.defect)
            for b in range(30):
                if b in sel:
                    continue
                for i, m in hist[b]:
                    who[m] = -2
                    nm -= 1
                    exits[i] = "matched_then_rotated_out"
        fo = np.array([w if w >= 0 else (-2 if w == -2 else -1) for w in who], np.int32)
        out = dict(nmatches=nm, frame_out=fo, point_match=np.array(pm, np.int32).reshape(-1), exit=exits,
                   tally=tallies)
        if kind == LOCAL:
            out["track"], out["track_level"] = self.track, self.level
        return out


def py_search(fr, pts, kind, th, nnratio=0.6, check_ori=True, mono=False, orb_dist=100, last_Tcw=None,
              frustum=False, limit=0.5, defect=None):
    """The reference's sequential scan.  who[f] is mvpMapPoints[f] during the call: -1 NULL, -3 a MapPoint
    that was there on entry, else the point that wrote it; obs[f]: that occupant has Observations() > 0."""
    S = Search(fr, pts, kind, th, nnratio, check_ori, mono, orb_dist, last_Tcw, frustum, limit, defect)
    occ = S.occ
    who = [(-3 if (occ is not None and occ[i]) else -1) for i in range(S.n)]
    if defect == "occ1_blocks_local":
        obs = [bool(occ is not None and occ[i] != 0) for i in range(S.n)]
    else:
        obs = [bool(occ is not None and occ[i] == 2) for i in range(S.n)]
    if kind in (LOCAL, LAST_FRAME):
        blocked = lambda idx: who[idx] not in (-1, -2) and obs[idx]  # noqa: E731
    elif kind == KEYFRAME:
        blocked = lambda idx: who[idx] not in (-1, -2)  # noqa: E731
    elif kind == SIM3:
        blocked = lambda idx: who[idx] != -1  # noqa: E731  vpMatched[idx]
    else:
        blocked = lambda idx: False  # noqa: E731
    pm, exits, tallies = [], [], []
    for i in range(S.npnt):
        m, code, tally = S.point(i, blocked)
        if m >= 0:
            who[m] = i
            obs[m] = bool(pts["flags"][i] & 2) or defect == "unflagged_blocks"
        pm.append(m)
        exits.append(code)
        tallies.append(tally)
    return S.finish(pm, exits, tallies, who)


def py_sweeps(fr, pts, kind, th, nnratio=0.6, check_ori=True, mono=False, orb_dist=100, last_Tcw=None,
              frustum=False, limit=0.5, defect=None):
    """The kernels' iteration: every point against the previous sweep's first-writer table (the smallest
    blocking point matched to each feature), the table rebuilt from the sweep's matches, until a sweep
    changes nothing.  The first sweep always counts as a change when there is a point; the kinds without
    an "already matched" state stop after it.  Returns py_search's dict plus `sweeps`, the number of
    sweeps evaluated, the confirming one included."""
    S = Search(fr, pts, kind, th, nnratio, check_ori, mono, orb_dist, last_Tcw, frustum, limit, defect)
    fw = [_INF] * S.n
    pm, sweeps = None, 0
    while True:
        res = [S.point(i, lambda idx, i=i: S.occupied(idx) or fw[idx] < i) for i in range(S.npnt)]
        new = [r[0] for r in res]
        changed = S.npnt > 0 and (sweeps == 0 or new != pm)
        sweeps += 1
        pm = new
        if not changed or kind in _FUSE_FAMILY:
            break
        fw = [_INF] * S.n
        for i, m in enumerate(pm):
            if m >= 0 and S.blocks(i):
                fw[m] = min(fw[m], i)
    who = [(-3 if (S.occ is not None and S.occ[f]) else -1) for f in range(S.n)]
    for i, m in enumerate(pm):
        if m >= 0:
            who[m] = i  # the last writer holds the feature
    out = S.finish(pm, [r[1] for r in res], [r[2] for r in res], who)
    out["sweeps"] = sweeps
    return out


# ------------------------------------------------------------------ SearchBySim3 (src/ORBmatcher.cc:1238-1487)
def sim3_pair(s12, R12, t12):
    """sR12 | t12 and sR21 | t21 as 4x4: s12*R12 and (1.0/s12)*R12.t() are convertTo(alpha); t21 = -sR21*t12
    is cv::gemm's small-matrix path with alpha = -1."""
    a12, a21 = f32(s12), f32(1.0 / float(s12))
    A12 = np.eye(4, dtype=np.float32)
    A21 = np.eye(4, dtype=np.float32)
    for r in range(3):
        for c in range(3):
            A12[r, c] = f32(R12[r, c] * a12)
            A21[r, c] = f32(R12[c, r] * a21)
        A12[r, 3] = t12[r]
    for r in range(3):
        t0 = f32(f32(A21[r, 0] * t12[0]) + f32(A21[r, 1] * t12[1]))
        A21[r, 3] = -f32(t0 + f32(A21[r, 2] * t12[2]))
    return A12, A21


def py_sim3_direction(own, other, pts, A, th, defect=None):
    """One direction of SearchBySim3: the MapPoints of KeyFrame `own` (one per feature) into KeyFrame
    `other` through A = [sR | t].  The result dict of py_search (kind BY_SIM3), exit codes included."""
    fr = dict(other, Tcw=np.asarray(own["Tcw"], np.float32), occ=None)
    return py_search(fr, pts, BY_SIM3, th, last_Tcw=A, defect=defect)


def py_search_by_sim3(kf1, kf2, pts1, pts2, s12, R12, t12, th, defect=None):
    """SearchBySim3 restated statement by statement (src/ORBmatcher.cc:1238-1487)."""
    A12, A21 = sim3_pair(s12, np.asarray(R12, np.float32), np.asarray(t12, np.float32))
    m1 = py_sim3_direction(kf1, kf2, pts1, A21, th, defect)["point_match"]
    m2 = py_sim3_direction(kf2, kf1, pts2, A12, th, defect)["point_match"]
    match12 = np.full(len(kf1["desc"]), -1, np.int32)
    for i1, idx2 in enumerate(m1):
        if idx2 >= 0 and m2[idx2] == i1:
            match12[i1] = idx2
    return int((match12 >= 0).sum()), match12

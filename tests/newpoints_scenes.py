"""Small CreateNewMapPoints problems for tests/test_newpoints.py: at most 64 features per keyframe
(320 for the compaction's block edge) and 1-3 neighbours, each built so that the pairs the search finds
are known by construction: a pair's two features share a FeatureVector node of their own and a
descriptor, every other descriptor is far away.

SCENES maps a name to (builder, claims).  A claim is what the literal must report for the scene:
  exits      set of pair exit codes that must occur (EXIT_NAMES)
  skips      tuple of the per-neighbour skip codes (SKIP_NAMES)
  n_new      accepted points in all
  done       neighbours_done
BOUNDARIES lists pairs of scenes that differ in one value set on either side of a threshold and must
end differently.  tests/test_newpoints.py checks on the CPU that the claims hold, that every exit and
skip code is claimed, that the libm variant of cos / atan2 decides every scene alike, and that every
defect of the literal changes at least one scene's result.

Some scenes need keyframe matrices no tracker would hand over (a singular "rotation", level sigmas of
1e30 that switch a gate off): the routine is arithmetic on its inputs, and these reach the exits
(`w == 0`, `dist == 0`) that rigid poses reach only by rounding luck.
"""
import numpy as np

from newpoints_literal import EXIT_NAMES, F32, SKIP_NAMES  # noqa: F401

F64 = np.float64
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
CAM = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, mb=0.5371657, mbf=386.1448)
DISTORT = (0.75, -0.5)  # mvKeys - mvKeysUn of every feature: what UnprojectStereo must read


def scale_factors(n=8, s=1.2):
    sf = np.ones(n, F32)
    for i in range(1, n):
        sf[i] = sf[i - 1] * F32(s)
    return sf


def pose(center, rot=(0.0, 0.0, 0.0)):
    """Tcw (float64) of a camera at `center` with small rotations about x, y, z."""
    ax, ay, az = rot
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ np.asarray(center, F64)
    return T


class Scene:
    def __init__(self, poses, monocular=False, cams=None, cur_pose=None):
        self.mono = monocular
        self.T = [np.eye(4) if cur_pose is None else np.asarray(cur_pose, F64)] + [np.asarray(p, F64) for p in poses]
        self.cam = [dict(CAM) for _ in self.T]
        for k, c in (cams or {}).items():
            self.cam[k].update(c)
        self.f = [[] for _ in self.T]   # per keyframe: feature dicts
        self.sig = [None for _ in self.T]
        self.next_id = 1

    def project(self, k, Xw):
        T, c = self.T[k], self.cam[k]
        Xc = T[:3, :3] @ np.asarray(Xw, F64) + T[:3, 3]
        return c["fx"] * Xc[0] / Xc[2] + c["cx"], c["fy"] * Xc[1] / Xc[2] + c["cy"], Xc[2]

    def feat(self, k, x, y, ident, octave=0, ur=-1.0, depth=-1.0, has_mp=0, mp_pos=(0, 0, 0)):
        self.f[k].append(dict(x=x, y=y, id=ident, octave=octave, ur=ur, depth=depth, has_mp=has_mp, mp_pos=mp_pos))
        return len(self.f[k]) - 1

    def obs(self, k, Xw, ident, octave=0, stereo=False, depth=None, d=(0.0, 0.0), ur_err=0.0, has_mp=0):
        """A feature of keyframe k observing Xw (+ pixel offset d); stereo: mvuRight / mvDepth from the true
        depth, or from `depth`."""
        u, v, z = self.project(k, Xw)
        if depth is not None:
            z = depth
        ur, dep = (-1.0, -1.0)
        if stereo:
            ur, dep = u + d[0] - self.cam[k]["mbf"] / z + ur_err, z
        return self.feat(k, u + d[0], v + d[1], ident, octave, ur, dep, has_mp, Xw)

    def pair(self, j, Xw, o1=0, o2=0, st1=False, st2=False, z1=None, z2=None, d1=(0.0, 0.0), d2=(0.0, 0.0),
             ur_err1=0.0, ur_err2=0.0, ident=None):
        """One feature of the current keyframe and one of neighbour j (0-based) that the search pairs."""
        if ident is None:
            ident = self.next_id
            self.next_id += 1
        i1 = self.obs(0, Xw, ident, o1, st1, z1, d1, ur_err1)
        i2 = self.obs(j + 1, Xw, ident, o2, st2, z2, d2, ur_err2)
        return i1, i2, ident

    def mappoint(self, j, Xw):
        """A feature of neighbour j that already holds a MapPoint at Xw (ComputeSceneMedianDepth)."""
        ident = self.next_id
        self.next_id += 1
        return self.obs(j + 1, Xw, ident, has_mp=1)

    def kf(self, k):
        fs, c = self.f[k], self.cam[k]
        n = len(fs)
        keys = np.zeros(n, KEYPOINT_DTYPE)
        keys["x"], keys["y"] = [f["x"] for f in fs], [f["y"] for f in fs]
        keys["octave"] = [f["octave"] for f in fs]
        keys["size"], keys["class_id"] = 31, -1
        ids = np.array([f["id"] for f in fs], np.int64)
        desc = np.zeros((n, 32), np.uint8)
        for i, ident in enumerate(ids):
            desc[i] = np.random.default_rng(1000 + int(ident)).integers(0, 256, 32, dtype=np.uint8)
        uniq = np.unique(ids)
        order = np.argsort(ids, kind="stable")
        counts = np.array([(ids == u).sum() for u in uniq], np.int64)
        sf = scale_factors()
        sig = (sf * sf).astype(F32) if self.sig[k] is None else np.asarray(self.sig[k], F32)
        xy = np.stack([keys["x"] + F32(DISTORT[0]), keys["y"] + F32(DISTORT[1])], axis=1).astype(F32)
        return dict(keys_un=keys, desc=desc, u_right=np.array([f["ur"] for f in fs], F32),
                    has_mp=np.array([f["has_mp"] for f in fs], np.uint8), node_id=uniq.astype(np.uint32),
                    node_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), feat=order.astype(np.int32),
                    keys_xy=xy, depth=np.array([f["depth"] for f in fs], F32),
                    mp_pos=np.array([f["mp_pos"] for f in fs], F32).reshape(n, 3), Tcw=self.T[k].astype(F32),
                    fx=F32(c["fx"]), fy=F32(c["fy"]), cx=F32(c["cx"]), cy=F32(c["cy"]), mb=F32(c["mb"]),
                    mbf=F32(c["mbf"]), scale_factors=sf, level_sigma2=sig)

    def problem(self):
        return dict(current=self.kf(0), neighbours=[self.kf(k) for k in range(1, len(self.T))],
                    monocular=self.mono, scale_factor=F32(1.2))


SIDE = pose((0.9, 0.0, 0.3), (0.01, -0.02, 0.005))      # a sideways step: high parallax
SIDE2 = pose((-0.8, 0.1, 0.4), (-0.01, 0.015, 0.0))
SIDE3 = pose((1.7, -0.1, 0.2), (0.0, -0.03, 0.01))
FWD = pose((0.0, 0.0, 0.9), (0.002, 0.001, 0.0))        # a forward step: low parallax near the axis


def grid_points(n, z0=8.0, z1=14.0):
    """n scene points spread over the image of the identity camera."""
    out = []
    for k in range(n):
        u, v = 80 + (k * 97) % 1080, 30 + (k * 53) % 300
        z = z0 + (z1 - z0) * ((k * 37) % 101) / 100.0
        out.append(((u - CAM["cx"]) * z / CAM["fx"], (v - CAM["cy"]) * z / CAM["fy"], z))
    return out


# ------------------------------------------------------------------ the scenes
def s_basic():
    """Triangulated pairs, mono and stereo, and both sides of the scale gate."""
    s = Scene([SIDE])
    s.pair(0, (1.0, 0.5, 10.0))
    s.pair(0, (-2.0, 1.0, 8.0), st1=True)
    s.pair(0, (2.0, -0.5, 9.0), st2=True)
    s.pair(0, (0.5, 0.2, 12.0), o1=0, o2=4)   # ratioOctave 0.48: above
    s.pair(0, (-0.5, 0.3, 12.0), o1=4, o2=0)  # ratioOctave 2.07: below
    return s.problem()


def s_behind():
    """A point behind both cameras (z1 <= 0) and one between them (z2 <= 0)."""
    s = Scene([SIDE, pose((0.0, 0.0, 12.0))])
    s.pair(0, (1.0, 0.5, -10.0))
    s.pair(1, (1.0, 0.0, 10.0))
    return s.problem()


def s_unproject(z_wrong=None, st2_too=False, ur_err=0.0):
    """A forward step: the rays' parallax is below the stereo parallax, so the depth is used."""
    def build():
        s = Scene([FWD])
        s.pair(0, (0.6, 0.3, 10.0), st1=True)                    # unprojected from the current keyframe
        s.pair(0, (-0.5, 0.2, 9.0), st2=True)                    # ... from the neighbour
        s.pair(0, (0.5, 0.2, 10.0))                              # neither is stereo: low parallax
        _, i2, _ = s.pair(0, (0.4, -0.3, 11.0), st1=True, st2=True)
        s.f[1][i2]["depth"] = 0.5                                # `else if`: KF2's (wrong) depth is not read
        if z_wrong is not None:
            s.pair(0, (0.6, -0.2, 10.0), st1=True, z1=z_wrong, st2=st2_too)   # KF1's depth is wrong
            s.pair(0, (-0.6, -0.2, 10.0), st2=True, z2=z_wrong)               # KF2's depth is wrong
        if ur_err:
            s.pair(0, (0.3, 0.35, 10.0), st1=True, st2=True, z1=5.0, ur_err2=ur_err)
        return s.problem()
    return build


def s_reproj_stereo():
    """Triangulated stereo pairs whose right coordinate disagrees (gates :487 and :514); the neighbour's
    mbf differs from the current keyframe's, and its stereo features agree with the CURRENT one (:509)."""
    s = Scene([SIDE], cams={1: dict(mbf=0.5 * CAM["mbf"])})
    s.pair(0, (1.0, 0.5, 10.0), st1=True, ur_err1=5.0)
    s.pair(0, (-1.0, 0.5, 10.0), st2=True, ur_err2=5.0)
    i1, i2, _ = s.pair(0, (-2.0, -0.5, 9.0), st2=True)
    f = s.f[1][i2]
    f["ur"] = f["x"] - CAM["mbf"] / f["depth"]   # consistent under mpCurrentKeyFrame->mbf
    return s.problem()


def s_reproj_mono():
    """A triangulated mono pair with the neighbour's keypoint off the epipolar line: a coarse level in KF2
    lets the search take it, a fine one in KF1 makes :476 refuse it.  (The search's own 3.84 sigma2 bound
    on the same keypoint keeps a triangulated pair from reaching :503; the wrong-depth scenes do.)"""
    s = Scene([SIDE])
    s.pair(0, (1.0, 0.5, 10.0), o1=0, o2=7, d2=(0.0, 7.0))
    return s.problem()


def s_depth_guard():
    s = Scene([FWD])
    i1, _, _ = s.pair(0, (0.6, 0.3, 10.0), st1=True)
    s.f[0][i1]["depth"] = 0.0
    _, i2, _ = s.pair(0, (-0.6, 0.3, 10.0), st2=True)
    s.f[1][i2]["depth"] = -1.0
    return s.problem()


def s_w_zero():
    """x3D(3) == 0: the neighbour's matrix has row 0 = x2 * row 2 (x2 = 0.25 exactly), so column 3 of A
    is orthogonal to the others, is never rotated, and a null vector with a zero last entry is sorted
    last.  Level sigmas of 1e30 keep the search from refusing the pair."""
    T2 = np.zeros((4, 4))
    T2[:3, :3] = [[0, 0, 0.25], [0, 1, 0], [0, 0, 1]]
    T2[:3, 3] = [100.0, 0, 0]
    T2[3, 3] = 1
    s = Scene([T2], cams={1: dict(fx=512.0, fy=512.0, cx=256.0, cy=128.0, mb=0.0)})
    s.feat(0, CAM["cx"] + 0.5 * CAM["fx"], CAM["cy"] + 0.25 * CAM["fy"], 1)
    s.feat(1, 384.0, 192.0, 1)
    s.sig[1] = np.full(8, 1e30, F32)
    return s.problem()


def s_dist_zero(rot):
    """dist2 == 0: the neighbour's feature has a depth of 1e-30, so UnprojectStereo returns its camera
    centre exactly; the rotation is one whose rounding leaves z2 > 0."""
    def build():
        s = Scene([pose((0.3, 0.1, 2.0), rot)])
        s.pair(0, (0.6, 0.3, 10.0), st2=True)
        f = s.f[1][0]
        f["depth"], f["ur"] = 1e-30, 0.0
        s.sig[0] = np.full(8, 1e30, F32)
        s.sig[1] = np.full(8, 1e30, F32)
        return s.problem()
    return build


def s_chain(n_nb=3):
    """Every scene point is seen by all neighbours: what neighbour 0 accepts, neighbour 1 must not search."""
    def build():
        s = Scene([SIDE, SIDE2, SIDE3][:n_nb])
        for k, X in enumerate(grid_points(12)):
            i1, _, ident = s.pair(0, X, st1=(k % 3 == 0))
            for j in range(1, n_nb):
                s.obs(j + 1, X, ident)
        # refused in neighbour 0 (scale gate), accepted in neighbour 1
        i1, _, ident = s.pair(0, (0.5, 0.2, 12.0), o1=0, o2=4)
        if n_nb > 1:
            s.obs(2, (0.5, 0.2, 12.0), ident)
        return s.problem()
    return build


def s_count(n_acc, n_feat=None):
    """n_acc accepted points in one neighbour (the compaction's wave and block edges), among refused ones."""
    def build():
        s = Scene([SIDE])
        n = n_feat or max(n_acc, 1)
        pts = grid_points(n)
        for k in range(n):
            if k < n_acc:
                s.pair(0, pts[k], st1=(k % 4 == 1))
            elif k % 2:
                s.pair(0, pts[k], o1=0, o2=4)      # matched, refused by the scale gate
            else:
                s.obs(0, pts[k], 5000 + k)         # unmatched
        if n_acc == 0:
            s.obs(1, pts[0], 7000)
        order = np.random.default_rng(n_acc).permutation(len(s.f[0]))   # accepted ones not contiguous
        s.f[0] = [s.f[0][i] for i in order]
        return s.problem()
    return build


def s_baseline(mb_bits):
    """The stereo gate: pKF2->mb one float below / at / above the baseline."""
    def build():
        import newpoints_literal as lit
        s = Scene([SIDE])
        s.pair(0, (1.0, 0.5, 10.0))
        p = s.problem()
        b = lit.gate(p, 0)["baseline"]
        mb = b
        for _ in range(abs(mb_bits)):
            mb = np.nextafter(mb, F32(np.inf if mb_bits > 0 else -np.inf))
        p["neighbours"][0]["mb"] = F32(mb)
        return p
    return build


def s_mono(depth_scale=1.0, with_points=True):
    """Monocular: the baseline / median-depth gate.  depth_scale moves neighbour 1's MapPoints away."""
    def build():
        s = Scene([SIDE, SIDE2], monocular=True)
        for k, X in enumerate(grid_points(9)):
            s.pair(0, X)
            s.pair(1, (X[0] + 0.1, X[1], X[2] + 1))
        if with_points:
            for X in grid_points(7, 9.0, 13.0):
                s.mappoint(0, X)
            for X in grid_points(6, 9.0, 13.0):   # an even count: rank (6-1)/2 = 2
                s.mappoint(1, tuple(depth_scale * np.asarray(X)))
        p = s.problem()
        for K in [p["current"]] + p["neighbours"]:
            K["u_right"][:] = -1
            K["depth"][:] = -1
        return p
    return build


def s_mono_ratio(bits):
    """The monocular gate at its threshold: neighbour 0 holds one MapPoint whose depth is set so that
    baseline/median lands `bits` floats from the first ratio whose double value is >= 0.01."""
    def build():
        import newpoints_literal as lit
        s = Scene([pose((0.9, 0.0, 0.0))], monocular=True)
        s.pair(0, (1.0, 0.5, 10.0))
        s.mappoint(0, (0.0, 0.0, 50.0))
        p = s.problem()
        K2 = p["neighbours"][0]
        K2["u_right"][:], K2["depth"][:] = -1, -1
        p["current"]["u_right"][:], p["current"]["depth"][:] = -1, -1
        b = lit.gate(p, 0)["baseline"]
        # the identity rotation: z of the MapPoint is its world z exactly; walk z to the threshold
        z = F32(b / F32(0.01))
        while F64(b / z) < 0.01:
            z = np.nextafter(z, F32(0))
        while F64(b / np.nextafter(z, F32(np.inf))) >= 0.01:
            z = np.nextafter(z, F32(np.inf))
        for _ in range(abs(bits)):   # bits < 0: towards a larger depth, a smaller ratio
            z = np.nextafter(z, F32(np.inf if bits < 0 else 0))
        i = int(np.nonzero(K2["has_mp"])[0][0])
        K2["mp_pos"][i] = (0.0, 0.0, z)
        return p
    return build


def s_z_zero(depth1):
    """z1 == 0 exactly: the current keyframe (no rotation, so Ow = -tcw exactly) has a stereo feature
    whose depth of 1e-30 makes UnprojectStereo return its own camera centre."""
    def build():
        s = Scene([SIDE], cur_pose=pose((0.2, 0.1, 0.3)))
        i1, _, _ = s.pair(0, (1.0, 0.5, 10.0), st1=True)
        s.f[0][i1]["depth"] = depth1
        return s.problem()
    return build


# ---- one-parameter families for the thresholds: bisect() walks the parameter to the two adjacent
# floats between which the literal's result changes
def f_sigma(scene, kf, pair_only=None):
    """level_sigma2[0] of keyframe kf (0: current) of a scene: the reprojection gates' 5.991 / 7.8 sigma2."""
    def build(v):
        p = SCENES_BASE[scene]()
        K = p["current"] if kf == 0 else p["neighbours"][kf - 1]
        K["level_sigma2"] = K["level_sigma2"].copy()
        K["level_sigma2"][0] = F32(v)
        return p
    return build


def f_scale_factor(o1, o2):
    """mfScaleFactor (ratioFactor = 1.5f * it) for one pair of levels o1, o2: the two sides of :534."""
    def build(v):
        s = Scene([SIDE])
        s.pair(0, (0.5, 0.2, 12.0), o1=o1, o2=o2)
        p = s.problem()
        p["scale_factor"] = F32(v)
        return p
    return build


def f_parallax(v):
    """A mono pair under a forward step, v its world x: cosParallaxRays against 0.9998."""
    s = Scene([FWD])
    s.pair(0, (v, 0.2, 10.0))
    return s.problem()


def f_stereo_parallax(v):
    """A stereo feature of the current keyframe under a sideways step, v its mvDepth:
    cosParallaxRays against cosParallaxStereo."""
    s = Scene([SIDE])
    i1, _, _ = s.pair(0, (-2.0, 1.0, 8.0), st1=True)
    s.f[0][i1]["depth"] = v
    return s.problem()


def signature(r, with_pos=False):
    """What a scene decides; with_pos: and the bits of the points it makes."""
    sig = (tuple(int(c) for c in r["exit"].ravel()), tuple(int(c) for c in r["nb_skip"]), int(r["n_new"]))
    return sig + (r["pos"].tobytes(),) if with_pos else sig


def bisect(build, lo, hi, run):
    """The adjacent float32 values lo < hi of a family between which run(build(v))'s signature changes
    (the family's ends must differ; the result is monotone in between)."""
    lo, hi = F32(lo), F32(hi)
    s_lo = signature(run(build(lo)))
    assert s_lo != signature(run(build(hi)))
    while np.nextafter(lo, hi) != hi:
        mid = F32((F64(lo) + F64(hi)) / 2)
        if mid == lo or mid == hi:
            break
        if signature(run(build(mid))) == s_lo:
            lo = mid
        else:
            hi = mid
    return lo, hi


SCENES = {
    "basic": (s_basic, dict(exits={"triangulated", "ratio_above", "ratio_below"}, skips=("ran",), n_new=3, done=1)),
    "behind": (s_behind, dict(exits={"z1", "z2"}, skips=("ran", "ran"), n_new=0, done=2)),
    "unproject": (s_unproject(), dict(exits={"unproject1", "unproject2", "low_parallax"}, skips=("ran",), n_new=3,
                                      done=1)),
    "unproject_wrong_depth": (s_unproject(5.0), dict(exits={"unproject1", "unproject2", "low_parallax",
                                                            "reproj2_mono", "reproj1_mono"}, skips=("ran",),
                                                     n_new=3, done=1)),
    "unproject_wrong_depth_stereo2": (s_unproject(5.0, st2_too=True), dict(exits={"reproj2_stereo", "reproj1_mono"},
                                                                          skips=("ran",), n_new=3, done=1)),
    "reproj_stereo": (s_reproj_stereo, dict(exits={"reproj1_stereo", "reproj2_stereo", "triangulated"},
                                            skips=("ran",), n_new=1, done=1)),
    "reproj_mono": (s_reproj_mono, dict(exits={"reproj1_mono"}, skips=("ran",), n_new=0, done=1)),
    "depth_guard": (s_depth_guard, dict(exits={"depth_guard"}, skips=("ran",), n_new=0, done=1)),
    "w_zero": (s_w_zero, dict(exits={"w_zero"}, skips=("ran",), n_new=0, done=1)),
    "dist_zero": (s_dist_zero((0.016, -0.0189, 0.007)), dict(exits={"dist_zero"}, skips=("ran",), n_new=0, done=1)),
    "chain2": (s_chain(2), dict(exits={"triangulated", "ratio_above"}, skips=("ran", "ran"), n_new=13, done=2)),
    "chain3": (s_chain(3), dict(exits={"triangulated"}, skips=("ran", "ran", "ran"), n_new=13, done=3)),
    "count0": (s_count(0, 6), dict(exits={"ratio_above"}, skips=("ran",), n_new=0, done=1)),
    "count1": (s_count(1, 5), dict(exits={"triangulated"}, skips=("ran",), n_new=1, done=1)),
    "count63": (s_count(63, 64), dict(exits={"triangulated"}, skips=("ran",), n_new=63, done=1)),
    "count64": (s_count(64), dict(exits={"triangulated"}, skips=("ran",), n_new=64, done=1)),
    "count65": (s_count(65, 66), dict(exits={"triangulated"}, skips=("ran",), n_new=65, done=1)),
    "count257": (s_count(257, 320), dict(exits={"triangulated", "ratio_above"}, skips=("ran",), n_new=257, done=1)),
    "baseline_below": (s_baseline(+1), dict(exits=set(), skips=("baseline",), n_new=0, done=1)),
    "baseline_at": (s_baseline(0), dict(exits={"triangulated"}, skips=("ran",), n_new=1, done=1)),
    "mono": (s_mono(), dict(exits={"triangulated"}, skips=("ran", "ran"), n_new=18, done=2)),
    "mono_far": (s_mono(200.0), dict(exits={"triangulated"}, skips=("ran", "ratio"), n_new=9, done=2)),
    "mono_no_depths": (s_mono(with_points=False), dict(exits=set(), skips=("no_depths", "no_depths"), n_new=0,
                                                       done=2)),
    "mono_ratio_at": (s_mono_ratio(0), dict(exits={"triangulated"}, skips=("ran",), n_new=1, done=1)),
    "mono_ratio_below": (s_mono_ratio(-1), dict(exits=set(), skips=("ratio",), n_new=0, done=1)),
    "z_zero": (s_z_zero(1e-30), dict(exits={"z1"}, skips=("ran",), n_new=0, done=1)),
    "z_small": (s_z_zero(1e-3), dict(exits={"z2"}, skips=("ran",), n_new=0, done=1)),
}
SCENES_BASE = {k: v[0] for k, v in SCENES.items()}

# name -> (family, lo, hi, the exit code that appears on one side only)
FAMILIES = {
    "reproj1_mono": (f_sigma("reproj_mono", 0), 1.0, 100.0, "reproj1_mono"),
    "reproj1_stereo": (f_sigma("reproj_stereo", 0), 1.0, 100.0, "reproj1_stereo"),
    "reproj2_mono": (f_sigma("unproject_wrong_depth", 1), 1.0, 1e4, "reproj2_mono"),
    "reproj2_stereo": (f_sigma("unproject_wrong_depth_stereo2", 1), 1.0, 1e4, "reproj2_stereo"),
    "ratio_above": (f_scale_factor(0, 4), 1.2, 2.0, "ratio_above"),
    "ratio_below": (f_scale_factor(4, 0), 1.2, 2.0, "ratio_below"),
    "parallax_0.9998": (f_parallax, 0.5, 4.0, "low_parallax"),
    "parallax_stereo": (f_stereo_parallax, 0.5, 8.0, "triangulated"),
}

# (scene, stop) -> claims, on "chain3": stop(i) is CheckNewKeyFrames() before neighbour i > 0.  "before"
# = the flag is up when the call starts (the first neighbour still runs, :320).
STOPS = {
    "before": (lambda i: True, None, dict(done=1, skips=("ran", "stopped", "stopped"))),
    "after0": (lambda i: i >= 1, 0, dict(done=1, skips=("ran", "stopped", "stopped"))),
    "after1": (lambda i: i >= 2, 1, dict(done=2, skips=("ran", "ran", "stopped"))),
}

# pairs of scenes on either side of a threshold: their results must differ
BOUNDARIES = [("baseline_below", "baseline_at"), ("mono_ratio_below", "mono_ratio_at"), ("z_zero", "z_small")]

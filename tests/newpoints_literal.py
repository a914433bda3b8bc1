"""A literal Python restatement of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:281-558) with
ComputeF12 (:672-699), KeyFrame::SetPose (src/KeyFrame.cc:80-101), ComputeSceneMedianDepth
(:784-819), UnprojectStereo (:759-781) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:343-393)
-- the yardstick of tests/test_newpoints.py.  It is not the code under test and needs no GPU.

Every arithmetic step is one IEEE operation on numpy float32 / float64 values in the order OpenCV 3.2
evaluates the reference's expressions; the per-pair steps run elementwise over a neighbour's matched
pairs (masked where the control flow differs).  The OpenCV pieces (Jacobi SVD, Mat::inv, the gemm
paths, convertTo, norm, dot) are tests/initializer_literal.py's, the trigonometric twins
tests/sim3_literal.py's.  The choices:

* SetPose: Rwc = Rcw.t() is a Mat of its own, so Ow = -Rwc*tcw is gemm(Rwc, tcw, alpha = -1) with
  flags == 0: the small-matrix path, (float)(t0*-1.0 + 0.0).  vBaseline = Ow2 - Ow1 in float,
  baseline = (float)cv::norm.
* ComputeSceneMedianDepth: z = (float)(Rcw2.dot(x3Dw) + (double)zcw) with Mat::dot in double, over the
  features holding a MapPoint; the element of rank (n-1)/2 of the ascending sort;
  ratioBaselineDepth = baseline/median in float, compared with 0.01 in double.  An empty list
  (vDepths[(0-1)/2]) is undefined in the reference: the neighbour is skipped with a code of its own.
* ComputeF12: R12 = R1w*R2w.t() carries a transpose flag and leaves the small path
  (GEMMSingleMul<float,double>).  -R1w*R2w.t()*t2w+t1w folds to gemm(gemm(R1w, R2w.t(), alpha = -1),
  t2w, 1, t1w, 1): the inner product in double with (float)(sum*-1.0), the outer on the small path
  with the C term.  K1.t().inv()*t12x*R12*K2.inv() is evaluated as it is written:
  Mat::inv() of K1.t() and of K2 (the n == 3 special case, double adjugate), three small-path
  products left to right.  (OpenCV's MatExpr may instead fold inv()*m into cv::solve; parity with the
  genuine library is unpinned for this row as for the others.)
* xn = ((u - cx)*invfx, (v - cy)*invfy, 1) in float with invfx = 1.0f/fx; ray = Rwc*xn on the small
  path; cosParallaxRays = (float)(ray1.dot(ray2)/(norm(ray1)*norm(ray2))), all double inside.
* cos(2*atan2(mb/2, mvDepth)): DBoW2/TemplatedVocabulary.h, included through KeyFrame.h, says `using
  namespace std` at global scope, so with float arguments overload resolution takes
  std::atan2(float, float) and std::cos(float): a = atan2f(mb/2.0f, depth), t = 2.0f*a, cosf(t).  The
  library evaluates them as (float)atan2_det((double).., (double)..) and (float) of sincos_d((double)t)'s
  cosine, each rounded once; `trig="libm"` uses math.atan2 / math.cos rounded the same way (the
  decisions of every scene must not depend on which).
* `else if(bStereo2)` (:411): a stereo feature of the current keyframe never consults KF2's depth.
  cosParallaxStereo = std::min(c1, c2) = c2 < c1 ? c2 : c1.  cosParallaxRays < 0.9998 compares in double.
* Linear triangulation: x*Tcw.row(2) - Tcw.row(r) is addWeighted, (a*x + b*(-1.0f)) + 0.0f, a - b when
  x == 1; cv::SVD::compute on the 4x4 is JacobiSVDImpl_<float> on A^T, U skipped; vt.row(3);
  x3D(3) == 0 skips; x3D.rowRange(0,3)/w is convertTo(1.0/(double)w).
* UnprojectStereo reads the DISTORTED mvKeys: x = (u - cx)*z*invfx left to right in float;
  Rwc*x3Dc + Ow is gemm with a C term on the small path.  mvDepth <= 0 returns an empty Mat that the
  reference then dots (undefined): guarded with a code of its own, where the branch is taken.
* z, x, y = (float)(Rcw.row(k).dot(x3Dt) + (double)tcw(k)); invz = (float)(1.0/(double)z); the errors
  in float left to right; the gates compare (double)err2 with 5.991*(double)sigma2 / 7.8*(double)sigma2.
  The second stereo gate uses the CURRENT keyframe's mbf (:509).
* dist = (float)cv::norm(x3D - Ow); ratioDist, ratioOctave, both products of the gate in float.
* UpdateNormalAndDepth with the two observations: normal = normal + normali/cv::norm(normali) is
  addWeighted(normal, 1, normali, 1/norm): (a*1.0f + b*(float)(1.0/norm)) + 0.0f, from zeros (the sum
  of two terms is the same in either order of the observation map); mNormalVector = normal/2 is
  convertTo(0.5); mfMaxDistance = dist1*mvScaleFactors[level of KF1's keypoint], mfMinDistance =
  mfMaxDistance/mvScaleFactors[nLevels-1] of KF1.
* The search runs with ORBmatcher(0.6, false): no rotation check, bOnlyStereo = false.

`defect=` switches one token, for the scenes' mutation check:
  "mbf2" (KF2's mbf at :509), "if411" (`else if` -> `if` at :411), "lt" (`<=` -> `<` at both depth
  tests), "keys_un" (UnprojectStereo on mvKeysUn), "one_sided" (the ratio gate's upper side only),
  "no_chain" (every neighbour searches with the has_mp of the call's start).
"""
import math

import numpy as np

from initializer_literal import (F32, F64, _recip, dot3, gemm_double, gemm_small, inv3, jacobi_svd, norm3,
                                 scale)
from sim3_literal import atan2_det, sincos_d

NONE, TRIANGULATED, UNPROJECT1, UNPROJECT2, LOW_PARALLAX, W_ZERO, Z1, Z2 = range(8)
REPROJ1_MONO, REPROJ1_STEREO, REPROJ2_MONO, REPROJ2_STEREO, DIST_ZERO, RATIO_BELOW, RATIO_ABOVE, DEPTH_GUARD = \
    range(8, 16)
NB_RAN, NB_BASELINE, NB_RATIO, NB_NO_DEPTHS, NB_STOPPED = range(5)
EXIT_NAMES = ("none", "triangulated", "unproject1", "unproject2", "low_parallax", "w_zero", "z1", "z2",
              "reproj1_mono", "reproj1_stereo", "reproj2_mono", "reproj2_stereo", "dist_zero", "ratio_below",
              "ratio_above", "depth_guard")
SKIP_NAMES = ("ran", "baseline", "ratio", "no_depths", "stopped")
DEFECTS = ("mbf2", "if411", "lt", "keys_un", "one_sided", "no_chain")


def cos_stereo(mb, depth, trig="twin"):
    """cos(2*atan2(mb/2, depth)) in the float overloads, elementwise over depth."""
    half = float(F32(mb) / F32(2))
    out = np.zeros(len(depth), F32)
    for k, d in enumerate(np.asarray(depth, F32)):
        if trig == "twin":
            t = F32(2) * F32(atan2_det(half, float(d)))
            out[k] = F32(sincos_d(float(t))[1])
        else:
            t = F32(2) * F32(math.atan2(half, float(d)))
            out[k] = F32(math.cos(float(t)))
    return out


def set_pose(K):
    """KeyFrame::SetPose -> dict(Rcw, tcw, Rwc, Ow, invfx, invfy)."""
    Tcw = np.asarray(K["Tcw"], F32).reshape(4, 4)
    Rcw, tcw = Tcw[:3, :3].copy(), Tcw[:3, 3].copy()
    Rwc = Rcw.T.copy()
    Ow = gemm_small(Rwc, tcw.reshape(3, 1), alpha=-1.0).reshape(3)
    return dict(Rcw=Rcw, tcw=tcw, Rwc=Rwc, Ow=Ow, invfx=F32(1) / F32(K["fx"]), invfy=F32(1) / F32(K["fy"]))


def scene_median_depth(K2, P2):
    """ComputeSceneMedianDepth(2) -> (n, median or None)."""
    sel = np.nonzero(np.asarray(K2["has_mp"]))[0]
    if len(sel) == 0:
        return 0, None
    x = np.asarray(K2["mp_pos"], F32).reshape(-1, 3)[sel]
    z = (dot3(P2["Rcw"][2], x) + F64(P2["tcw"][2])).astype(F32)
    return len(sel), np.sort(z)[(len(sel) - 1) // 2]


def compute_f12(K1, P1, K2, P2):
    R12 = gemm_double(P1["Rcw"], P2["Rcw"], tb=True)
    M = gemm_double(P1["Rcw"], P2["Rcw"], alpha=-1.0, tb=True)
    t12 = gemm_small(M, P2["tcw"].reshape(3, 1), C=P1["tcw"].reshape(3, 1)).reshape(3)
    z = F32(0)
    tx = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], F32)
    K1t = np.array([[K1["fx"], 0, 0], [0, K1["fy"], 0], [K1["cx"], K1["cy"], 1]], F32)
    K2m = np.array([[K2["fx"], 0, K2["cx"]], [0, K2["fy"], K2["cy"]], [0, 0, 1]], F32)
    return gemm_small(gemm_small(gemm_small(inv3(K1t), tx), R12), inv3(K2m))


def _row(x, P, r):
    x = x[:, None]
    with np.errstate(all="ignore"):
        return np.where(x == 1, P[2][None, :] - P[r][None, :],
                        (P[2][None, :] * x + P[r][None, :] * F32(-1)) + F32(0)).astype(F32)


def _unproject(K, P, idx, z, defect):
    if defect == "keys_un" or K.get("keys_xy") is None:
        u, v = K["keys_un"]["x"][idx], K["keys_un"]["y"][idx]
    else:
        xy = np.asarray(K["keys_xy"], F32).reshape(-1, 2)
        u, v = xy[idx, 0], xy[idx, 1]
    with np.errstate(all="ignore"):
        xc = np.stack([(u - F32(K["cx"])) * z * P["invfx"], (v - F32(K["cy"])) * z * P["invfy"], z], axis=0).astype(F32)
        return gemm_small(P["Rwc"], xc, C=P["Ow"].reshape(3, 1)).T


def pairs(K1, P1, K2, P2, ratioFactor, i1, i2, defect=None, trig="twin"):
    """:383-556 of the matched pairs (i1[k], i2[k]) -> dict(code, cos [M, 3], X, normal, dist [M, 2])."""
    M = len(i1)
    out = dict(code=np.zeros(M, np.uint8), cos=np.zeros((M, 3), F32), X=np.zeros((M, 3), F32),
               normal=np.zeros((M, 3), F32), dist=np.zeros((M, 2), F32))
    if M == 0:
        return out
    kp1, kp2 = K1["keys_un"][i1], K2["keys_un"][i2]
    ur1 = np.asarray(K1["u_right"], F32)[i1] if K1.get("u_right") is not None else np.full(M, -1, F32)
    ur2 = np.asarray(K2["u_right"], F32)[i2] if K2.get("u_right") is not None else np.full(M, -1, F32)
    d1 = np.asarray(K1["depth"], F32)[i1] if K1.get("depth") is not None else np.full(M, -1, F32)
    d2 = np.asarray(K2["depth"], F32)[i2] if K2.get("depth") is not None else np.full(M, -1, F32)
    st1, st2 = ur1 >= 0, ur2 >= 0
    fx1, fy1, cx1, cy1 = (F32(K1[k]) for k in ("fx", "fy", "cx", "cy"))
    fx2, fy2, cx2, cy2 = (F32(K2[k]) for k in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        one = np.ones(M, F32)
        xn1 = np.stack([(kp1["x"] - cx1) * P1["invfx"], (kp1["y"] - cy1) * P1["invfy"], one], axis=0).astype(F32)
        xn2 = np.stack([(kp2["x"] - cx2) * P2["invfx"], (kp2["y"] - cy2) * P2["invfy"], one], axis=0).astype(F32)
        ray1, ray2 = gemm_small(P1["Rwc"], xn1).T, gemm_small(P2["Rwc"], xn2).T
        cosr = (dot3(ray1, ray2) / (norm3(ray1) * norm3(ray2))).astype(F32)
        cs = cosr + F32(1)
        c1 = np.where(st1, cos_stereo(K1["mb"], d1, trig), cs).astype(F32)
        use2 = st2 if defect == "if411" else (~st1 & st2)
        c2 = np.where(use2, cos_stereo(K2["mb"], d2, trig), cs).astype(F32)
        cst = np.where(c2 < c1, c2, c1)
        tri = (cosr < cst) & (cosr > 0) & (st1 | st2 | (cosr.astype(F64) < 0.9998))
        un1 = ~tri & st1 & (c1 < c2)
        un2 = ~tri & ~un1 & st2 & (c2 < c1)
        code = np.where(tri, TRIANGULATED, np.where(un1, UNPROJECT1, np.where(un2, UNPROJECT2, LOW_PARALLAX)))
        alive = code != LOW_PARALLAX
        # linear triangulation
        T1, T2 = np.asarray(K1["Tcw"], F32).reshape(4, 4), np.asarray(K2["Tcw"], F32).reshape(4, 4)
        A = np.stack([_row(xn1[0], T1, 0), _row(xn1[1], T1, 1), _row(xn2[0], T2, 0), _row(xn2[1], T2, 1)], axis=1)
        _, _, Vt = jacobi_svd(np.swapaxes(A, 1, 2), 0)
        x = Vt[:, 3, :]
        Xt = scale(x[:, :3], (F64(1) / x[:, 3].astype(F64))[:, None])
        X = np.where(tri[:, None], Xt, np.where(un1[:, None], _unproject(K1, P1, i1, d1, defect),
                                                _unproject(K2, P2, i2, d2, defect))).astype(F32)

        def leave(mask, c):
            nonlocal code, alive
            m = alive & mask
            code = np.where(m, c, code)
            alive = alive & ~m

        leave(tri & (x[:, 3] == 0), W_ZERO)
        leave((un1 & ~(d1 > 0)) | (un2 & ~(d2 > 0)), DEPTH_GUARD)
        z1 = (dot3(P1["Rcw"][2], X) + F64(P1["tcw"][2])).astype(F32)
        leave((z1 < 0) if defect == "lt" else (z1 <= 0), Z1)
        z2 = (dot3(P2["Rcw"][2], X) + F64(P2["tcw"][2])).astype(F32)
        leave((z2 < 0) if defect == "lt" else (z2 <= 0), Z2)
        sig1 = np.asarray(K1["level_sigma2"], F32)[kp1["octave"]].astype(F64)
        x1 = (dot3(P1["Rcw"][0], X) + F64(P1["tcw"][0])).astype(F32)
        y1 = (dot3(P1["Rcw"][1], X) + F64(P1["tcw"][1])).astype(F32)
        iz1 = _recip(z1)
        u1, v1 = fx1 * x1 * iz1 + cx1, fy1 * y1 * iz1 + cy1
        ex, ey = u1 - kp1["x"], v1 - kp1["y"]
        er = (u1 - F32(K1["mbf"]) * iz1) - ur1
        leave(~st1 & ((ex * ex + ey * ey).astype(F64) > 5.991 * sig1), REPROJ1_MONO)
        leave(st1 & ((ex * ex + ey * ey + er * er).astype(F64) > 7.8 * sig1), REPROJ1_STEREO)
        sig2 = np.asarray(K2["level_sigma2"], F32)[kp2["octave"]].astype(F64)
        x2 = (dot3(P2["Rcw"][0], X) + F64(P2["tcw"][0])).astype(F32)
        y2 = (dot3(P2["Rcw"][1], X) + F64(P2["tcw"][1])).astype(F32)
        iz2 = _recip(z2)
        u2, v2 = fx2 * x2 * iz2 + cx2, fy2 * y2 * iz2 + cy2
        ex, ey = u2 - kp2["x"], v2 - kp2["y"]
        mbf = F32(K2["mbf"]) if defect == "mbf2" else F32(K1["mbf"])
        er = (u2 - mbf * iz2) - ur2
        leave(~st2 & ((ex * ex + ey * ey).astype(F64) > 5.991 * sig2), REPROJ2_MONO)
        leave(st2 & ((ex * ex + ey * ey + er * er).astype(F64) > 7.8 * sig2), REPROJ2_STEREO)
        n1v, n2v = X - P1["Ow"][None, :], X - P2["Ow"][None, :]
        n1d, n2d = norm3(n1v), norm3(n2v)
        dist1, dist2 = n1d.astype(F32), n2d.astype(F32)
        leave((dist1 == 0) | (dist2 == 0), DIST_ZERO)
        sf1, sf2 = np.asarray(K1["scale_factors"], F32), np.asarray(K2["scale_factors"], F32)
        ratioDist = dist2 / dist1
        ratioOctave = sf1[kp1["octave"]] / sf2[kp2["octave"]]
        rf = F32(ratioFactor)
        if defect != "one_sided":
            leave(ratioDist * rf < ratioOctave, RATIO_BELOW)
        leave(ratioDist > ratioOctave * rf, RATIO_ABOVE)
        b1, b2 = (F64(1) / n1d).astype(F32)[:, None], (F64(1) / n2d).astype(F32)[:, None]
        s1 = (F32(0) * F32(1) + n1v * b1) + F32(0)
        s2 = (s1 * F32(1) + n2v * b2) + F32(0)
        dmax = dist1 * sf1[kp1["octave"]]
        dmin = dmax / sf1[len(sf1) - 1]
        out["code"] = code.astype(np.uint8)
        out["cos"] = np.stack([cosr, c1, c2], axis=1).astype(F32)
        out["X"] = X
        out["normal"] = scale(s2.astype(F32), F64(0.5))
        out["dist"] = np.stack([dmin, dmax], axis=1).astype(F32)
    return out


def gate(P, i):
    """The head of the loop body for neighbour i -> dict(skip, baseline, median, F12, P1, P2)."""
    K1, K2 = P["current"], P["neighbours"][i]
    P1, P2 = set_pose(K1), set_pose(K2)
    baseline = norm3(P2["Ow"] - P1["Ow"]).astype(F32)
    skip, median = NB_RAN, F32(0)
    if not P["monocular"]:
        if baseline < F32(K2["mb"]):
            skip = NB_BASELINE
    else:
        n, med = scene_median_depth(K2, P2)
        if n == 0:
            skip = NB_NO_DEPTHS
        else:
            median = med
            with np.errstate(all="ignore"):
                if F64(baseline / median) < 0.01:
                    skip = NB_RATIO
    F12 = compute_f12(K1, P1, K2, P2) if skip == NB_RAN else np.zeros((3, 3), F32)
    return dict(skip=skip, baseline=baseline, median=median, F12=F12, P1=P1, P2=P2)


def search_problem(K1, K2, g, has_mp1):
    """The dict tests/test_triangulation.py py_triangulation (or oracle.search_for_triangulation) takes."""
    kf1 = {k: K1[k] for k in ("keys_un", "desc", "u_right", "node_id", "node_off", "feat")}
    kf1["has_mp"] = has_mp1
    kf2 = {k: K2[k] for k in ("keys_un", "desc", "u_right", "has_mp", "node_id", "node_off", "feat")}
    return dict(kf1=kf1, kf2=kf2, F12=g["F12"], C1w=g["P1"]["Ow"], T2w=np.asarray(K2["Tcw"], F32).reshape(4, 4),
                fx=F32(K2["fx"]), fy=F32(K2["fy"]), cx=F32(K2["cx"]), cy=F32(K2["cy"]),
                scale_factors2=np.asarray(K2["scale_factors"], F32),
                level_sigma2_2=np.asarray(K2["level_sigma2"], F32))


def create_new_map_points(P, search, stop=None, defect=None, trig="twin"):
    """The neighbour loop.  search(pr) -> (nmatches, match12) is SearchForTriangulation(.., false) of a
    matcher without the rotation check; stop(i) is CheckNewKeyFrames() before neighbour i > 0."""
    K1 = P["current"]
    n1, nn = len(K1["desc"]), len(P["neighbours"])
    has0 = np.asarray(K1["has_mp"], np.uint8).copy()
    has_mp1 = has0.copy()
    ratioFactor = F32(1.5) * F32(P["scale_factor"])
    R = dict(points=[], pos=[], normal=[], dist=[], nb_skip=np.full(nn, NB_STOPPED, np.int32),
             nb_nmatches=np.zeros(nn, np.int32), nb_baseline=np.zeros(nn, F32), nb_median=np.zeros(nn, F32),
             exit=np.zeros((nn, n1), np.uint8), cos=np.zeros((nn, n1, 3), F32), F12=np.zeros((nn, 3, 3), F32),
             match12=np.full((nn, n1), -1, np.int32), neighbours_done=0)
    for i in range(nn):
        if i > 0 and stop is not None and stop(i):
            break
        R["neighbours_done"] = i + 1
        K2 = P["neighbours"][i]
        g = gate(P, i)
        R["nb_skip"][i], R["nb_baseline"][i], R["nb_median"][i], R["F12"][i] = g["skip"], g["baseline"], g["median"], g["F12"]
        if g["skip"] != NB_RAN:
            continue
        _, m12 = search(search_problem(K1, K2, g, has0 if defect == "no_chain" else has_mp1))
        m12 = np.asarray(m12, np.int32)
        i1 = np.nonzero(m12 >= 0)[0]
        i2 = m12[i1]
        R["match12"][i], R["nb_nmatches"][i] = m12, len(i1)
        o = pairs(K1, g["P1"], K2, g["P2"], ratioFactor, i1, i2, defect, trig)
        R["exit"][i, i1], R["cos"][i, i1] = o["code"], o["cos"]
        for k in np.nonzero((o["code"] >= TRIANGULATED) & (o["code"] <= UNPROJECT2))[0]:
            R["points"].append((i, int(i1[k]), int(i2[k])))
            R["pos"].append(o["X"][k])
            R["normal"].append(o["normal"][k])
            R["dist"].append(o["dist"][k])
            has_mp1[i1[k]] = 1
    n = len(R["points"])
    R["n_new"] = n
    R["points"] = np.array(R["points"], np.int32).reshape(n, 3)
    for k, w in (("pos", 3), ("normal", 3), ("dist", 2)):
        R[k] = np.array(R[k], F32).reshape(n, w)
    R["has_mp1"] = has_mp1
    return R

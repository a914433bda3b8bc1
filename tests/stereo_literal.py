"""A literal restatement of Frame::ComputeStereoMatches (reference src/Frame.cc:547-788), statement by
statement, with one exit code per left keypoint.  It pins oracle_stereo_match (oracle/orb_oracle.cpp),
which is written in the kernel's structure; this file follows the reference's.

Arithmetic.  Every value the reference holds in a `float` is an np.float32 here and every operation on
floats rounds to float once, as the compiled reference does:

* mvScaleFactors / mvInvScaleFactors are the extractor's tables (src/ORBextractor.cc:427-441): a float
  vector filled with products by the DOUBLE member scaleFactor, and 1.0f / scale.
* `r = 2.0f * scale`, `ceil(kpY + r)`, `floor(kpY - r)`: float sum, then the int conversion.
* `vRowIndices[vL]` converts the float row to an index by truncation.
* `round` is C round (half away from zero), on the float product `pt * scaleFactor`.
* `cv::norm(IL, IR, NORM_L1)` of the two centred CV_32F patches: every pixel and every centred
  difference is an integer of magnitude <= 510, the sum at most 121 * 510 = 61710, so each float or
  double partial sum is exact and `float dist` holds the exact integer.
* `dist < bestDist` compares the float with the int converted to float (INT_MAX -> 2147483648.f);
  `bestDist = dist` truncates (exact here).
* deltaR, bestuR, disparity: float operations in the reference's order.
* The clamp is literal: `disparity = 0.01` stores the double constant to a float (0.01f);
  `bestuR = uL - 0.01` is computed in DOUBLE and rounded once to float.  (The oracle and the kernel
  compute uL - 0.01f in float; tests/test_stereo_literal.py checks that the two agree wherever a clamp
  can occur.)
* `median = vDistIdx[size/2].first` int -> float; `thDist = 1.5f * 1.4f * median`, i.e.
  (1.5f * 1.4f) * median in float; `first < thDist` compares int -> float.

Guards.  In three places the reference's behaviour is undefined; the literal states the guards that the
oracle states (and the library implements):

1. A band row outside [0, nRows): `vRowIndices[yi].push_back` for yi < 0 or yi >= nRows writes out of
   bounds.  Guard: rows outside are skipped (the band is clamped).
2. A `rowRange` / `colRange` that leaves the level: cv::Mat asserts (an exception no caller handles).
   Guard: the keypoint is left unmatched (exit `guard`).  The reference forms the left patch before the
   `endu` test and the right windows after it; the literal keeps that order, so a left patch that leaves
   the level is `guard` even when `endu` would fire as well.
3. An empty vDistIdx: `vDistIdx[vDistIdx.size()/2]` reads element 0 of an empty vector.  Guard: nothing
   is filtered.

Unreachable exits.  The literal asserts that it never takes them.

* `maxU < 0` (:624): minD == 0, so maxU == uL, and a keypoint has uL >= 0.
* `deltaR < -1 || deltaR > 1` (:738): bestincR is the FIRST strict minimum of the eleven SADs and is
  interior here (the `edgeinc` exit came before), so d1 > d2 (a strictly smaller or equal earlier value
  would have been kept instead) and d3 >= d2.  With a = d1 - d2 > 0 and b = d3 - d2 >= 0,
  deltaR = (a - b) / (2 (a + b)) and |a - b| <= a + b, so |deltaR| <= 0.5.  All SADs are integers
  <= 61710, so d1 - d3, d1 + d3 and 2 d2 (< 2^24) are exact in float and the only rounding is the
  final division, which cannot carry 0.5 past 1.

Exit codes (one per left keypoint):
  norow    vRowIndices[vL] is empty
  orb      best Hamming distance >= thOrbDist (75), which includes "no candidate passed the filters"
  endu     iniu < 0 || endu >= cols
  guard    a patch leaves the level (guard 2)
  edgeinc  bestincR == -L or +L
  neg      disparity < minD
  far      disparity >= maxD
  clamp    accepted with disparity <= 0 (stored as 0.01)
  ok       accepted
`median[i]` marks an accepted match (clamp / ok) that the final filter removes.
"""
import math

import numpy as np

F32 = np.float32
TH_HIGH, TH_LOW = 100, 50  # src/ORBmatcher.cc:37-38
EXITS = ("norow", "orb", "endu", "guard", "edgeinc", "neg", "far", "clamp", "ok")
INT_MAX = 2 ** 31 - 1


def scale_factors(scale_factor, nlevels):
    """mvScaleFactor / mvInvScaleFactor (src/ORBextractor.cc:427-441): the ctor's float argument kept in a
    double member; each entry the float of (previous entry as double) * member."""
    sf = float(F32(scale_factor))
    scale = [F32(1.0)]
    for _ in range(1, nlevels):
        scale.append(F32(float(scale[-1]) * sf))
    inv = [F32(1.0) / s for s in scale]
    return scale, inv


def c_round(x):
    """C round() of a float: half away from zero (the result is exact in float for |x| < 2^23)."""
    x = float(x)
    return F32(math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5))


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1844-1860): the bit count of a ^ b over 256 bits."""
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def compute_stereo_matches(scale_factor, nlevels, kL, dL, kR, dR, pyrL, pyrR, bf, baseline):
    """kL / kR: keypoint records (fields x, y, octave); dL / dR: uint8 [n, 32]; pyrL / pyrR: the
    extractors' mvImagePyramid (lists of 2-D uint8 arrays).  Returns a dict: uRight, depth (float32),
    sad (int32, -1 unless accepted), exit (list of str), median (bool array), nmatches."""
    N = len(kL)
    mvScaleFactors, mvInvScaleFactors = scale_factors(scale_factor, nlevels)
    mbf, mb = F32(bf), F32(baseline)
    mvuRight = np.full(N, -1.0, F32)
    mvDepth = np.full(N, -1.0, F32)
    sad_out = np.full(N, -1, np.int32)
    exits = [None] * N
    thOrbDist = (TH_HIGH + TH_LOW) // 2
    nRows = pyrL[0].shape[0]
    vRowIndices = [[] for _ in range(nRows)]
    Nr = len(kR)
    for iR in range(Nr):
        kpY = F32(kR["y"][iR])
        r = F32(2.0) * mvScaleFactors[int(kR["octave"][iR])]
        maxr = int(math.ceil(float(kpY + r)))
        minr = int(math.floor(float(kpY - r)))
        for yi in range(minr, maxr + 1):
            if yi < 0 or yi >= nRows:  # guard 1
                continue
            vRowIndices[yi].append(iR)
    minZ = mb
    minD = F32(0)
    maxD = mbf / minZ
    vDistIdx = []
    for iL in range(N):
        levelL = int(kL["octave"][iL])
        vL, uL = F32(kL["y"][iL]), F32(kL["x"][iL])
        vCandidates = vRowIndices[int(vL)]
        if not vCandidates:
            exits[iL] = "norow"
            continue
        minU = uL - maxD
        maxU = uL - minD
        assert not maxU < 0, "unreachable: maxU < 0"
        bestDist = TH_HIGH
        bestIdxR = 0
        for iR in vCandidates:
            octR = int(kR["octave"][iR])
            if octR < levelL - 1 or octR > levelL + 1:
                continue
            uR = F32(kR["x"][iR])
            if uR >= minU and uR <= maxU:
                dist = descriptor_distance(dL[iL], dR[iR])
                if dist < bestDist:
                    bestDist = dist
                    bestIdxR = iR
        if not bestDist < thOrbDist:
            exits[iL] = "orb"
            continue
        uR0 = F32(kR["x"][bestIdxR])
        scaleFactor = mvInvScaleFactors[levelL]
        scaleduL = c_round(uL * scaleFactor)
        scaledvL = c_round(vL * scaleFactor)
        scaleduR0 = c_round(uR0 * scaleFactor)
        w = 5
        imL, imR = pyrL[levelL], pyrR[levelL]
        rows, cols = imL.shape
        r0, r1 = int(scaledvL - F32(w)), int(scaledvL + F32(w) + F32(1))
        c0, c1 = int(scaleduL - F32(w)), int(scaleduL + F32(w) + F32(1))
        if r0 < 0 or r1 > rows or c0 < 0 or c1 > cols:  # guard 2, left patch
            exits[iL] = "guard"
            continue
        IL = imL[r0:r1, c0:c1].astype(F32)
        IL = IL - IL[w, w]
        bestDist = INT_MAX
        bestincR = 0
        L = 5
        vDists = [F32(0)] * (2 * L + 1)
        iniu = scaleduR0 + F32(L) - F32(w)
        endu = scaleduR0 + F32(L) + F32(w) + F32(1)
        if iniu < 0 or endu >= F32(imR.shape[1]):
            exits[iL] = "endu"
            continue
        left_ok = True
        for incR in range(-L, L + 1):
            q0 = int(scaleduR0 + F32(incR) - F32(w))
            q1 = int(scaleduR0 + F32(incR) + F32(w) + F32(1))
            if q0 < 0 or q1 > imR.shape[1]:  # guard 2, right window
                left_ok = False
                break
            IR = imR[r0:r1, q0:q1].astype(F32)
            IR = IR - IR[w, w]
            exact = int(np.abs(IL.astype(np.int64) - IR.astype(np.int64)).sum())
            dist = F32(exact)
            assert int(dist) == exact
            if dist < F32(bestDist):
                bestDist = int(dist)
                bestincR = incR
            vDists[L + incR] = dist
        if not left_ok:
            exits[iL] = "guard"
            continue
        if bestincR == -L or bestincR == L:
            exits[iL] = "edgeinc"
            continue
        dist1, dist2, dist3 = vDists[L + bestincR - 1], vDists[L + bestincR], vDists[L + bestincR + 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            deltaR = (dist1 - dist3) / (F32(2.0) * (dist1 + dist3 - F32(2.0) * dist2))
        assert not (deltaR < -1 or deltaR > 1), "unreachable: |deltaR| > 1"
        bestuR = mvScaleFactors[levelL] * (scaleduR0 + F32(bestincR) + deltaR)
        disparity = uL - bestuR
        if disparity >= minD and disparity < maxD:
            code = "ok"
            if disparity <= 0:
                disparity = F32(0.01)
                bestuR = F32(float(uL) - 0.01)
                code = "clamp"
            mvDepth[iL] = mbf / disparity
            mvuRight[iL] = bestuR
            vDistIdx.append((bestDist, iL))
            sad_out[iL] = bestDist
            exits[iL] = code
        else:
            exits[iL] = "neg" if disparity < minD else "far"
    median_flag = np.zeros(N, bool)
    if vDistIdx:  # guard 3
        vDistIdx.sort()
        median = F32(vDistIdx[len(vDistIdx) // 2][0])
        thDist = F32(1.5) * F32(1.4) * median
        for i in range(len(vDistIdx) - 1, -1, -1):
            if F32(vDistIdx[i][0]) < thDist:
                break
            mvuRight[vDistIdx[i][1]] = -1
            mvDepth[vDistIdx[i][1]] = -1
            median_flag[vDistIdx[i][1]] = True
    assert all(e in EXITS for e in exits)
    return {"uRight": mvuRight, "depth": mvDepth, "sad": sad_out, "exit": exits, "median": median_flag,
            "nmatches": len(vDistIdx) - int(median_flag.sum())}

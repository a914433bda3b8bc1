"""A literal Python restatement of the reference's Initializer (src/Initializer.cc:40-1345) -- the
yardstick of tests/test_initializer.py and tests/test_initializer_shim.py.  It is not the code under
test and needs no GPU.

Every arithmetic step is one IEEE operation on numpy float32 / float64 values, in the order OpenCV
3.2 evaluates the reference's expressions.  Loops over hypotheses and over matches run the same
single operations elementwise on arrays (masked where the control flow differs per element); every
accumulated sum is a Python loop in the reference's order.  The choices:

* cv::SVDecomp / cv::SVD::compute on CV_32F is JacobiSVDImpl_<float> on the generic (non-SIMD) path,
  restated as oracle/pnp.cpp restates the double instantiation: float matrix entries and float c, s
  (each rounded from a double expression), W and the sd / p / a / b / beta / gamma / delta sums in
  double, minval = FLT_MIN, eps = 2 FLT_EPSILON, hypot(p, beta) written sqrt(p*p + beta*beta),
  max(m, 30) sweeps.  _SVDcompute: m >= n works on A^T (n rows of length m); m < n (8x9) works on A's
  rows with n1 = 9, so vt.row(8) is the basis completion from cv::RNG(0x12345678): +-1/9 by bit 8
  of RNG::next(), two Gram-Schmidt passes (float products summed in double, the update rounded to
  float, a float L1 sum, 1/asum when asum > 100 eps), then normalised by (float)(1/sd).  The same
  completion runs for every row of a 3x3 whose singular value is <= FLT_MIN.  Outputs nobody reads
  are skipped: U of the 16x9 and of the 4x4 (so their completion too), V of the 8x9.
* Mat::inv() of a 3x3 CV_32F: the n == 3 special case, the determinant and the adjugate in double,
  t = (double)(..) * (1/det), rounded to float; det == 0 gives the zero matrix.
* cv::determinant of a 3x3 CV_32F: det3 in double.
* cv::norm(NORM_L2) of 3 floats: sqrt of a double sum of squares in order.  Mat::dot of 3 floats:
  double products summed in order.
* A*B with flags == 0 and 3x3 / 3x1 results is cv::gemm's small-matrix path: a float dot product
  left to right, then (float)(t0*alpha + 0.0) in double, or (float)(t0*alpha + c*beta) with a C.
  K*P2 (3x3 by 3x4), K.t()*F, u*W.t() and -R.t()*t leave that path: GEMMSingleMul<float,double>,
  the products summed in double from 0 in order, (float)(sum*alpha).
* MatExpr scalings (t/norm(t), x/w, tp *= d, -t, -R) are convertTo(alpha): x*(float)alpha + 0.0f,
  a plain copy when |alpha - 1| < DBL_EPSILON.  s*U*Rp*Vt is gemm(gemm(U, Rp, alpha = s), Vt).
  x*P.row(2) - P.row(0) is addWeighted: (a*x + b*(-1.0f)) + 0.0f, or a - b when x == 1.
* Normalize runs over all keypoints of a frame with float accumulators in index order.
* Check* sum the score in float in match order, two conditional adds per match; 1.0/(..) terms are
  double divisions rounded to float.  `currentScore > score`: the first best hypothesis wins.
* FindFundamental's mask stays empty when no hypothesis scores above 0 (reported as all false).
* acos is the float overload: acosf_det, (float)atan2_det(sqrt((1 - x)(1 + x)), x) in double, shared
  with the library; parallax = (float)((double)(acosf*180.0f) / CV_PI).
* Degenerate inputs, where the reference's source does not determine its behaviour: fewer than 8
  matches is an argument error (ValueError); SH = SF = 0 returns false with `degenerate` set; NaN
  cosines sort after every number (std::sort on NaN is undefined), as numpy.sort does.

`Initializer.rec` keeps what a stage-by-stage comparison needs.
"""
import math

import numpy as np

from sim3_literal import atan2_det

F32 = np.float32
F64 = np.float64
RAND_MAX = 2147483647
FLT_MIN = F64(np.finfo(F32).tiny)
SVD_EPS = F32(np.finfo(F32).eps * 2)
DBL_EPSILON = 2.220446049250313e-16
CV_PI = F64(3.1415926535897932384626433832795)


def acosf_det(x, atan2=atan2_det):
    """Python twin of orbx_device.h acosf_det."""
    x = F32(x)
    if x == 0:
        x = F32(0)
    xd = F64(x)
    with np.errstate(all="ignore"):
        y = np.sqrt((F64(1) - xd) * (F64(1) + xd))
    return F32(atan2(float(y), float(xd)))


def acosf_libm(x):
    """math.acos rounded to float (the decisions of a run must not depend on which acos it uses)."""
    x = float(F32(x))
    return F32(math.acos(x)) if -1.0 <= x <= 1.0 else F32("nan")


# ------------------------------------------------------------------ OpenCV 3.2 pieces
def _rng_next(state):
    state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & 0xFFFFFFFFFFFFFFFF
    return state, state & 0xFFFFFFFF


def _complete_row(A, i, m, sd, state):
    """The basis completion of JacobiSVDImpl_ for row i of one matrix A [rows, m] (float32, in
    place); returns (sd, rng state)."""
    val0 = F32(1.0 / m)
    thr = SVD_EPS * F32(100)
    for _ in range(100):
        if not sd <= FLT_MIN:
            break
        for k in range(m):
            state, r = _rng_next(state)
            A[i, k] = val0 if (r & 256) != 0 else -val0
        for _it in range(2):
            for j in range(i):
                sd = F64(0)
                for k in range(m):
                    sd = sd + F64(A[i, k] * A[j, k])
                asum = F32(0)
                for k in range(m):
                    t = F32(F64(A[i, k]) - sd * F64(A[j, k]))
                    A[i, k] = t
                    asum = asum + abs(t)
                asum = F32(1) / asum if asum > thr else F32(0)
                for k in range(m):
                    A[i, k] = A[i, k] * asum
        sd = F64(0)
        for k in range(m):
            t = F64(A[i, k])
            sd = sd + t * t
        sd = np.sqrt(sd)
    return sd, state


def jacobi_svd(At, n1, with_v=True):
    """JacobiSVDImpl_<float> on a batch.  At: [B, n, m] float32, n rows of length m.  Returns
    (At [B, max(n, n1), m], w [B, n] float32, Vt [B, n, n] or None).  Vt is treated as present in
    the control flow even when with_v is False (its arithmetic is skipped because nobody reads it)."""
    At = np.array(At, F32, copy=True)
    B, n, m = At.shape
    if n1 > n:
        At = np.concatenate([At, np.zeros((B, n1 - n, m), F32)], axis=1)
    ar = np.arange(B)
    W = np.zeros((B, n), F64)
    with np.errstate(all="ignore"):
        for i in range(n):
            sd = np.zeros(B, F64)
            for k in range(m):
                t = At[:, i, k].astype(F64)
                sd = sd + t * t
            W[:, i] = sd
        Vt = np.tile(np.eye(n, dtype=F32), (B, 1, 1)) if with_v else None
        for _ in range(max(m, 30)):
            changed = False
            for i in range(n - 1):
                for j in range(i + 1, n):
                    Ai, Aj = At[:, i, :], At[:, j, :]
                    a, b = W[:, i], W[:, j]
                    p = np.zeros(B, F64)
                    for k in range(m):
                        p = p + Ai[:, k].astype(F64) * Aj[:, k].astype(F64)
                    rot = ~(np.abs(p) <= F64(SVD_EPS) * np.sqrt(a * b))
                    if not rot.any():
                        continue
                    p = p * F64(2)
                    beta = a - b
                    gamma = np.sqrt(p * p + beta * beta)
                    delta = (gamma - beta) * F64(0.5)
                    s_n = np.sqrt(delta / gamma).astype(F32)
                    c_n = (p / (gamma * s_n.astype(F64) * F64(2))).astype(F32)
                    c_p = np.sqrt((gamma + beta) / (gamma * F64(2))).astype(F32)
                    s_p = (p / (gamma * c_p.astype(F64) * F64(2))).astype(F32)
                    neg = beta < 0
                    c = np.where(neg, c_n, c_p)[:, None]
                    s = np.where(neg, s_n, s_p)[:, None]
                    t0 = c * Ai + s * Aj
                    t1 = (-s) * Ai + c * Aj
                    na, nb = np.zeros(B, F64), np.zeros(B, F64)
                    for k in range(m):
                        na = na + t0[:, k].astype(F64) * t0[:, k].astype(F64)
                        nb = nb + t1[:, k].astype(F64) * t1[:, k].astype(F64)
                    At[:, i, :] = np.where(rot[:, None], t0, Ai)
                    At[:, j, :] = np.where(rot[:, None], t1, Aj)
                    W[:, i] = np.where(rot, na, a)
                    W[:, j] = np.where(rot, nb, b)
                    changed = True
                    if with_v:
                        Vi, Vj = Vt[:, i, :], Vt[:, j, :]
                        v0 = c * Vi + s * Vj
                        v1 = (-s) * Vi + c * Vj
                        Vt[:, i, :] = np.where(rot[:, None], v0, Vi)
                        Vt[:, j, :] = np.where(rot[:, None], v1, Vj)
            if not changed:
                break
        for i in range(n):
            sd = np.zeros(B, F64)
            for k in range(m):
                t = At[:, i, k].astype(F64)
                sd = sd + t * t
            W[:, i] = np.sqrt(sd)
        for i in range(n - 1):
            j = np.full(B, i)
            for k in range(i + 1, n):
                j = np.where(W[ar, j] < W[:, k], k, j)
            sw = np.nonzero(j != i)[0]
            if len(sw):
                js = j[sw]
                W[sw, i], W[sw, js] = W[sw, js].copy(), W[sw, i].copy()
                At[sw, i], At[sw, js] = At[sw, js].copy(), At[sw, i].copy()
                if with_v:
                    Vt[sw, i], Vt[sw, js] = Vt[sw, js].copy(), Vt[sw, i].copy()
        w = W.astype(F32)
        states = [0x12345678] * B
        for i in range(n1):
            sd = W[:, i].copy() if i < n else np.zeros(B, F64)
            for bi in np.nonzero(sd <= FLT_MIN)[0]:
                sd[bi], states[bi] = _complete_row(At[bi], i, m, sd[bi], states[bi])
            s = np.where(sd > FLT_MIN, F64(1) / sd, F64(0)).astype(F32)
            At[:, i, :] = At[:, i, :] * s[:, None]
    return At, w, Vt


def svd_square(A):
    """cv::SVD::compute(A, w, u, vt, FULL_UV) of [B, n, n] CV_32F: (u, w, vt)."""
    A = np.asarray(A, F32)
    n = A.shape[-1]
    At, w, Vt = jacobi_svd(np.swapaxes(A, 1, 2), n)
    return np.swapaxes(At[:, :n, :], 1, 2).copy(), w, Vt


def _f2d(x):
    return np.asarray(x, F32).astype(F64)


def det3(M):
    m = _f2d(M)
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1]) -
            m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0]) +
            m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))


def inv3(M):
    """Mat::inv() (DECOMP_LU) of [..., 3, 3] CV_32F."""
    S = _f2d(M)
    with np.errstate(all="ignore"):
        d = det3(M)
        ok = d != 0
        d = F64(1) / d
        idx = [((1, 1), (2, 2), (1, 2), (2, 1)), ((0, 2), (2, 1), (0, 1), (2, 2)), ((0, 1), (1, 2), (0, 2), (1, 1)),
               ((1, 2), (2, 0), (1, 0), (2, 2)), ((0, 0), (2, 2), (0, 2), (2, 0)), ((0, 2), (1, 0), (0, 0), (1, 2)),
               ((1, 0), (2, 1), (1, 1), (2, 0)), ((0, 1), (2, 0), (0, 0), (2, 1)), ((0, 0), (1, 1), (0, 1), (1, 0))]
        out = np.zeros(S.shape, F32)
        for k, (a, b, c, e) in enumerate(idx):
            t = (S[(Ellipsis,) + a] * S[(Ellipsis,) + b] - S[(Ellipsis,) + c] * S[(Ellipsis,) + e]) * d
            out[..., k // 3, k % 3] = np.where(ok, t, F64(0)).astype(F32)
    return out


def gemm_small(A, B, alpha=1.0, C=None):
    """cv::gemm's small-matrix path for [..., 3, 3] x [..., 3, c]: float dot product left to right,
    then (float)(t0*alpha + c*beta) in double (beta = 1 with a C, c = 0 without)."""
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    with np.errstate(all="ignore"):
        t0 = (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + \
            A[..., :, 2, None] * B[..., None, 2, :]
        add = F64(0) if C is None else _f2d(C) * F64(1)
        return (t0.astype(F64) * np.asarray(alpha, F64) + add).astype(F32)


def gemm_double(A, B, alpha=1.0, ta=False, tb=False):
    """GEMMSingleMul<float,double>: sum_k (double)a(i,k) * (double)b(k,j) from 0 in order, (float)(sum*alpha)."""
    A, B = _f2d(A), _f2d(B)
    if ta:
        A = np.swapaxes(A, -1, -2)
    if tb:
        B = np.swapaxes(B, -1, -2)
    with np.errstate(all="ignore"):
        s = np.zeros(A.shape[:-1] + B.shape[-1:], F64)
        for k in range(A.shape[-1]):
            s = s + A[..., :, k, None] * B[..., None, k, :]
        return (s * F64(alpha)).astype(F32)


def scale(x, alpha):
    """convertTo(alpha): x*(float)alpha + 0.0f, a copy when |alpha - 1| < DBL_EPSILON.  alpha: double(s)."""
    x = np.asarray(x, F32)
    alpha = np.asarray(alpha, F64)
    with np.errstate(all="ignore"):
        return np.where(np.abs(alpha - F64(1)) < DBL_EPSILON, x, x * alpha.astype(F32) + F32(0)).astype(F32)


def norm3(v):
    """cv::norm of [..., 3] floats, a double."""
    v = _f2d(v)
    with np.errstate(all="ignore"):
        s = np.zeros(v.shape[:-1], F64)
        for k in range(3):
            s = s + v[..., k] * v[..., k]
        return np.sqrt(s)


def dot3(a, b):
    a, b = _f2d(a), _f2d(b)
    with np.errstate(all="ignore"):
        s = np.zeros(a.shape[:-1], F64)
        for k in range(3):
            s = s + a[..., k] * b[..., k]
        return s


def _recip(x):
    """(float)(1.0 / x) for float x."""
    with np.errstate(all="ignore"):
        return (F64(1) / np.asarray(x, F32).astype(F64)).astype(F32)


# ------------------------------------------------------------------ the reference's functions
def normalize(keys):
    """Normalize (:1076-1131) -> (vNormalizedPoints [n, 2], T [3, 3])."""
    keys = np.asarray(keys, F32).reshape(-1, 2)
    n = len(keys)
    with np.errstate(all="ignore"):
        mx, my = F32(0), F32(0)
        for i in range(n):
            mx = mx + keys[i, 0]
            my = my + keys[i, 1]
        mx, my = mx / F32(n), my / F32(n)
        P = np.stack([keys[:, 0] - mx, keys[:, 1] - my], axis=1).astype(F32)
        dx, dy = F32(0), F32(0)
        Pa = np.abs(P)
        for i in range(n):
            dx = dx + Pa[i, 0]
            dy = dy + Pa[i, 1]
        dx, dy = dx / F32(n), dy / F32(n)
        sx, sy = _recip(dx), _recip(dy)
        P = np.stack([P[:, 0] * sx, P[:, 1] * sy], axis=1).astype(F32)
        T = np.eye(3, dtype=F32)
        T[0, 0], T[1, 1], T[0, 2], T[1, 2] = sx, sy, (-mx) * sx, (-my) * sy
    return P, T


def compute_h21(P1, P2):
    """ComputeH21 (:315-360) of [B, 8, 2] normalised point sets -> [B, 3, 3]."""
    P1, P2 = np.asarray(P1, F32), np.asarray(P2, F32)
    B = len(P1)
    u1, v1, u2, v2 = P1[..., 0], P1[..., 1], P2[..., 0], P2[..., 1]
    A = np.zeros((B, 16, 9), F32)
    A[:, 0::2, 3], A[:, 0::2, 4], A[:, 0::2, 5] = -u1, -v1, F32(-1)
    A[:, 0::2, 6], A[:, 0::2, 7], A[:, 0::2, 8] = v2 * u1, v2 * v1, v2
    A[:, 1::2, 0], A[:, 1::2, 1], A[:, 1::2, 2] = u1, v1, F32(1)
    A[:, 1::2, 6], A[:, 1::2, 7], A[:, 1::2, 8] = (-u2) * u1, (-u2) * v1, -u2
    _, _, Vt = jacobi_svd(np.swapaxes(A, 1, 2), 0)
    return Vt[:, 8, :].reshape(B, 3, 3).copy()


def compute_f21(P1, P2):
    """ComputeF21 (:374-421) of [B, 8, 2] normalised point sets -> [B, 3, 3]."""
    P1, P2 = np.asarray(P1, F32), np.asarray(P2, F32)
    B = len(P1)
    u1, v1, u2, v2 = P1[..., 0], P1[..., 1], P2[..., 0], P2[..., 1]
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], axis=2).astype(F32)
    At, _, _ = jacobi_svd(A, 9, with_v=False)
    Fpre = At[:, 8, :].reshape(B, 3, 3)
    u, w, vt = svd_square(Fpre)
    D = np.zeros((B, 3, 3), F32)
    D[:, 0, 0], D[:, 1, 1] = w[:, 0], w[:, 1]
    return gemm_small(gemm_small(u, D), vt)


def check_homography(H21, H12, u1, v1, u2, v2, sigma):
    """CheckHomography (:424-533) of [B, 3, 3] models over the N matches -> (score [B], mask [B, N])."""
    th = F32(5.991)
    sigma = F32(sigma)
    inv_s2 = _recip(sigma * sigma)
    h, g = H21.reshape(-1, 9)[:, :, None], H12.reshape(-1, 9)[:, :, None]
    with np.errstate(all="ignore"):
        w2 = _recip(g[:, 6] * u2 + g[:, 7] * v2 + g[:, 8])
        x = (g[:, 0] * u2 + g[:, 1] * v2 + g[:, 2]) * w2
        y = (g[:, 3] * u2 + g[:, 4] * v2 + g[:, 5]) * w2
        chi1 = ((u1 - x) * (u1 - x) + (v1 - y) * (v1 - y)) * inv_s2
        w1 = _recip(h[:, 6] * u1 + h[:, 7] * v1 + h[:, 8])
        x = (h[:, 0] * u1 + h[:, 1] * v1 + h[:, 2]) * w1
        y = (h[:, 3] * u1 + h[:, 4] * v1 + h[:, 5]) * w1
        chi2 = ((u2 - x) * (u2 - x) + (v2 - y) * (v2 - y)) * inv_s2
        return _score(chi1, chi2, th, th)


def check_fundamental(F21, u1, v1, u2, v2, sigma):
    """CheckFundamental (:536-636)."""
    th, th_score = F32(3.841), F32(5.991)
    sigma = F32(sigma)
    inv_s2 = _recip(sigma * sigma)
    f = F21.reshape(-1, 9)[:, :, None]
    with np.errstate(all="ignore"):
        a2 = f[:, 0] * u1 + f[:, 1] * v1 + f[:, 2]
        b2 = f[:, 3] * u1 + f[:, 4] * v1 + f[:, 5]
        c2 = f[:, 6] * u1 + f[:, 7] * v1 + f[:, 8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2
        a1 = f[:, 0] * u2 + f[:, 3] * v2 + f[:, 6]
        b1 = f[:, 1] * u2 + f[:, 4] * v2 + f[:, 7]
        c1 = f[:, 2] * u2 + f[:, 5] * v2 + f[:, 8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2
        return _score(chi1, chi2, th, th_score)


def _score(chi1, chi2, th, th_score):
    out1, out2 = chi1 > th, chi2 > th
    score = np.zeros(chi1.shape[0], F32)
    t1, t2 = th_score - chi1, th_score - chi2
    for i in range(chi1.shape[1]):
        score = np.where(out1[:, i], score, score + t1[:, i])
        score = np.where(out2[:, i], score, score + t2[:, i])
    return score.astype(F32), ~(out1 | out2)


def sample_sets(rng, iterations, N):
    """The set loop of Initialize (:109-131) on a rand() stream: DUtils::Random::RandomInt + swap-remove."""
    sets = np.zeros((iterations, 8), np.int64)
    for it in range(iterations):
        avail = list(range(N))
        for j in range(8):
            randi = int((float(rng.rand()) / (float(RAND_MAX) + 1.0)) * len(avail))
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


def triangulate(kp1, kp2, P1, P2):
    """Triangulate (:1018-1064) of [M, 2] point pairs -> [M, 3]."""
    def row(x, P, r):
        x = x[:, None]
        with np.errstate(all="ignore"):
            return np.where(x == 1, P[2][None, :] - P[r][None, :],
                            (P[2][None, :] * x + P[r][None, :] * F32(-1)) + F32(0)).astype(F32)
    A = np.stack([row(kp1[:, 0], P1, 0), row(kp1[:, 1], P1, 1), row(kp2[:, 0], P2, 0), row(kp2[:, 1], P2, 1)], axis=1)
    _, _, Vt = jacobi_svd(np.swapaxes(A, 1, 2), 0)
    x = Vt[:, 3, :]
    with np.errstate(all="ignore"):
        return scale(x[:, :3], (F64(1) / x[:, 3].astype(F64))[:, None])


def check_rt(R, t, keys1, keys2, m1, m2, inliers, K, th2, acos=acosf_det):
    """CheckRT (:1134-1303) -> (nGood, vP3D [n1, 3], vbGood [n1], parallax)."""
    n1 = len(keys1)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    vbGood = np.zeros(n1, bool)
    vP3D = np.zeros((n1, 3), F32)
    P1 = np.zeros((3, 4), F32)
    P1[:, :3] = K
    P2 = np.zeros((3, 4), F32)
    P2[:, :3], P2[:, 3] = R, t
    P2 = gemm_double(K, P2)
    O2 = gemm_double(R, np.asarray(t, F32).reshape(3, 1), alpha=-1.0, ta=True).reshape(3)
    sel = np.nonzero(inliers)[0]
    if len(sel) == 0:
        return 0, vP3D, vbGood, F32(0)
    i1, i2 = m1[sel], m2[sel]
    kp1, kp2 = keys1[i1], keys2[i2]
    with np.errstate(all="ignore"):
        X = triangulate(kp1, kp2, P1, P2)
        alive = np.isfinite(X).all(axis=1)
        n1v = X - F32(0)
        dist1 = norm3(n1v).astype(F32)
        n2v = X - O2[None, :]
        dist2 = norm3(n2v).astype(F32)
        cosp = (dot3(n1v, n2v) / (dist1 * dist2).astype(F64)).astype(F32)
        low = cosp < F64(0.99998)
        alive &= ~((X[:, 2] <= 0) & low)
        X2 = gemm_small(R, X.T, C=np.asarray(t, F32).reshape(3, 1)).T
        alive &= ~((X2[:, 2] <= 0) & low)
        iz = _recip(X[:, 2])
        e1x, e1y = fx * X[:, 0] * iz + cx - kp1[:, 0], fy * X[:, 1] * iz + cy - kp1[:, 1]
        alive &= ~(e1x * e1x + e1y * e1y > th2)
        iz = _recip(X2[:, 2])
        e2x, e2y = fx * X2[:, 0] * iz + cx - kp2[:, 0], fy * X2[:, 1] * iz + cy - kp2[:, 1]
        alive &= ~(e2x * e2x + e2y * e2y > th2)
    nGood = int(alive.sum())
    vP3D[i1[alive]] = X[alive]
    vbGood[i1[alive & low]] = True
    if nGood > 0:
        cs = np.sort(cosp[alive])  # NaN after every number
        c = cs[min(50, nGood - 1)]
        with np.errstate(all="ignore"):
            parallax = F32(F64(acos(c) * F32(180)) / CV_PI)
    else:
        parallax = F32(0)
    return nGood, vP3D, vbGood, parallax


def decompose_e(E):
    """DecomposeE (:1317-1345) -> (R1, R2, t)."""
    u, _, vt = svd_square(E[None])
    u, vt = u[0], vt[0]
    t = u[:, 2].copy()
    with np.errstate(all="ignore"):
        t = scale(t, F64(1) / norm3(t))
    W = np.zeros((3, 3), F32)
    W[0, 1], W[1, 0], W[2, 2] = -1, 1, 1
    R1 = gemm_small(gemm_small(u, W), vt)
    if det3(R1) < 0:
        R1 = scale(R1, F64(-1))
    R2 = gemm_small(gemm_double(u, W, tb=True), vt)
    if det3(R2) < 0:
        R2 = scale(R2, F64(-1))
    return R1, R2, t


def decompose_h(H21, K):
    """The 8 motion hypotheses of ReconstructH (:792-929) -> (vR, vt) or None on the d1/d2, d2/d3 exit."""
    A = gemm_small(gemm_small(inv3(K), H21), K)
    U, w, Vt = svd_square(A[None])
    U, w, Vt = U[0], w[0], Vt[0]
    s = F32(det3(U) * det3(Vt))
    d1, d2, d3 = w[0], w[1], w[2]
    with np.errstate(all="ignore"):
        if F64(d1 / d2) < 1.00001 or F64(d2 / d3) < 1.00001:
            return None
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        st = [aux_st, -aux_st, -aux_st, aux_st]
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        vR, vt = [], []
        for i in range(8):
            Rp = np.eye(3, dtype=F32)
            if i < 4:
                Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ct, -st[i], st[i], ct
                tp = np.array([x1[i], 0, -x3[i]], F32)
                tp = scale(tp, F64(d1 - d3))
            else:
                j = i - 4
                Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cp, sp[j], -1, sp[j], -cp
                tp = np.array([x1[j], 0, x3[j]], F32)
                tp = scale(tp, F64(d1 + d3))
            vR.append(gemm_small(gemm_small(U, Rp, alpha=F64(s)), Vt))
            t = gemm_small(U, tp.reshape(3, 1)).reshape(3)
            vt.append(scale(t, F64(1) / norm3(t)))
    return vR, vt


class Initializer:
    """The reference class: Initializer(keys_un, K, sigma, iterations), Initialize(keys_un2,
    vMatches12, rng) -> (ok, R21, t21, vP3D, vbTriangulated); rng.rand() is the process rand()
    (the caller seeds it: SeedRandOnce(0) is the caller's stream)."""

    def __init__(self, keys_un, K, sigma=1.0, iterations=200, acos=acosf_det):
        self.mvKeys1 = np.ascontiguousarray(keys_un, F32).reshape(-1, 2)
        self.mK = np.ascontiguousarray(K, F32).reshape(3, 3)
        self.mSigma = F32(sigma)
        self.mSigma2 = F32(sigma) * F32(sigma)
        self.mMaxIterations = int(iterations)
        self.acos = acos
        self.rec = None

    def Initialize(self, keys_un2, vMatches12, rng):
        keys2 = np.ascontiguousarray(keys_un2, F32).reshape(-1, 2)
        vm = np.asarray(vMatches12, np.int64).reshape(-1)
        if len(vm) != len(self.mvKeys1):
            raise ValueError("Initializer: vMatches12 must have one entry per reference keypoint")
        m1 = np.nonzero(vm >= 0)[0]
        m2 = vm[m1]
        N = len(m1)
        if N < 8 or (m2 >= len(keys2)).any():
            raise ValueError("Initializer: fewer than 8 matches, or a match index out of range")
        its = self.mMaxIterations
        sets = sample_sets(rng, its, N)
        rec = {"N": N, "sets": sets, "degenerate": False, "n_hyp": 0, "nGood": np.zeros(8, np.int32),
               "parallax": np.zeros(8, F32), "ok": False, "model": -1}
        self.rec = rec
        k1, k2 = self.mvKeys1, keys2
        Pn1, T1 = normalize(k1)
        Pn2, T2 = normalize(k2)
        S1, S2 = Pn1[m1[sets]], Pn2[m2[sets]]
        u1, v1, u2, v2 = k1[m1, 0], k1[m1, 1], k2[m2, 0], k2[m2, 1]
        # FindHomography (:170-226)
        H21 = gemm_small(gemm_small(inv3(T2), compute_h21(S1, S2)), T1)
        H12 = inv3(H21)
        sH, mH = check_homography(H21, H12, u1, v1, u2, v2, self.mSigma)
        # FindFundamental (:229-294)
        F21 = gemm_small(gemm_small(T2.T.copy(), compute_f21(S1, S2)), T1)
        sF, mF = check_fundamental(F21, u1, v1, u2, v2, self.mSigma)
        rec["scoresH"], rec["scoresF"], rec["H21_all"], rec["F21_all"] = sH, sF, H21, F21

        def walk(sc):
            best, score = -1, F32(0)
            for it in range(its):
                if sc[it] > score:
                    best, score = it, sc[it]
            return best, score
        itH, SH = walk(sH)
        itF, SF = walk(sF)
        rec.update(SH=SH, SF=SF, itH=itH, itF=itF,
                   H21=H21[itH].copy() if itH >= 0 else np.zeros((3, 3), F32),
                   F21=F21[itF].copy() if itF >= 0 else np.zeros((3, 3), F32),
                   maskH=mH[itH].copy() if itH >= 0 else np.zeros(N, bool),
                   maskF=mF[itF].copy() if itF >= 0 else np.zeros(N, bool))
        fail = (False, None, None, None, None)
        if itH < 0 and itF < 0:
            rec["degenerate"] = True
            return fail
        with np.errstate(all="ignore"):
            RH = SH / (SH + SF)
        th2 = F32(F64(4.0) * F64(self.mSigma2))
        if F64(RH) > 0.40:
            rec["model"] = 0
            return self._reconstruct_h(rec, k1, k2, m1, m2, th2)
        rec["model"] = 1
        return self._reconstruct_f(rec, k1, k2, m1, m2, th2)

    def _check(self, rec, i, R, t, mask, k1, k2, m1, m2, th2):
        n, P, g, par = check_rt(R, t, k1, k2, m1, m2, mask, self.mK, th2, self.acos)
        rec["nGood"][i], rec["parallax"][i] = n, par
        return n, P, g, par

    def _reconstruct_f(self, rec, k1, k2, m1, m2, th2, minParallax=F32(1.0), minTriangulated=50):
        """ReconstructF (:648-763)."""
        mask = rec["maskF"]
        N = int(mask.sum())
        K = self.mK
        E21 = gemm_small(gemm_double(K, rec["F21"], ta=True), K)
        R1, R2, t = decompose_e(E21)
        t2 = scale(t, F64(-1))
        hyp = [(R1, t), (R2, t), (R1, t2), (R2, t2)]
        rec["n_hyp"] = 4
        rec["hyp"] = hyp
        res = [self._check(rec, i, R, tt, mask, k1, k2, m1, m2, th2) for i, (R, tt) in enumerate(hyp)]
        good = [r[0] for r in res]
        maxGood = max(good)
        nMinGood = max(int(0.9 * N), minTriangulated)
        nsimilar = sum(1 for g in good if g > 0.7 * maxGood)
        if maxGood < nMinGood or nsimilar > 1:
            rec["why"] = "ambiguous" if nsimilar > 1 else "few"
            return False, None, None, None, None
        i = good.index(maxGood)
        if res[i][3] > minParallax:
            rec["ok"] = True
            return True, hyp[i][0].copy(), hyp[i][1].copy(), res[i][1], res[i][2]
        rec["why"] = "parallax"
        return False, None, None, None, None

    def _reconstruct_h(self, rec, k1, k2, m1, m2, th2, minParallax=F32(1.0), minTriangulated=50):
        """ReconstructH (:776-983)."""
        mask = rec["maskH"]
        N = int(mask.sum())
        dec = decompose_h(rec["H21"], self.mK)
        if dec is None:
            rec["why"] = "singular_values"
            return False, None, None, None, None
        vR, vt = dec
        rec["n_hyp"] = 8
        rec["hyp"] = list(zip(vR, vt))
        bestGood, secondBestGood, bestIdx, bestParallax, best = 0, 0, -1, F32(-1), None
        for i in range(8):
            n, P, g, par = self._check(rec, i, vR[i], vt[i], mask, k1, k2, m1, m2, th2)
            if n > bestGood:
                secondBestGood, bestGood, bestIdx, bestParallax, best = bestGood, n, i, par, (P, g)
            elif n > secondBestGood:
                secondBestGood = n
        if secondBestGood < 0.75 * bestGood and bestParallax >= minParallax and bestGood > minTriangulated and \
                bestGood > 0.9 * N:
            rec["ok"] = True
            return True, vR[bestIdx].copy(), vt[bestIdx].copy(), best[0], best[1]
        rec["why"] = "ambiguous" if not secondBestGood < 0.75 * bestGood else \
            ("parallax" if not bestParallax >= minParallax else "few")
        return False, None, None, None, None

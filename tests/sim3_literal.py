"""A literal Python restatement of the reference's Sim3Solver (src/Sim3Solver.cc:37-481) -- the
yardstick of tests/test_sim3.py and tests/test_sim3_shim.py.  It is not the code under test and
needs no GPU.

Every arithmetic step is one IEEE operation on a numpy float32 / float64 scalar (the per-point
loops of CheckInliers / Project / FromCameraToImage run the same single operations elementwise on
arrays), in the order OpenCV 3.2 evaluates the reference's expressions:

* cv::reduce(P, C, 1, CV_REDUCE_SUM) of a 3-column CV_32F row: reduceC_'s two accumulators,
  (p0 + p2) + p1 in float; C/P.cols is convertTo(alpha = 1./3): x * (float)alpha + 0.0f.
* Pr2*Pr1.t() is the GEMM_2_T path, GEMMSingleMul<float,double>: the three products summed in
  double, rounded once to float.
* cv::eigen on the 4x4 CV_32F N is JacobiImpl_<float>: pivot by indR / indC, hypot rotations,
  eps = FLT_EPSILON, at most 30 n^2 sweeps, eigenvalues sorted descending with their rows.
* cv::norm is the square root of a double sum of squares; atan2 in double (atan2_det, shared with
  the library, or math.atan2).
* 2*ang*vec/norm(vec) is one MatExpr scale alpha = (2*ang) * (1./norm), applied by convertTo.
* cv::Rodrigues: double inside (theta < DBL_EPSILON -> identity; cos/sin through sincos_d, shared
  with the library), float in and out.
* mR12i*Pr2 and R*X + t are cv::gemm's small-matrix path: a float dot product left to right, then
  (float)(t0*alpha + c*beta) in double.
* Mat::dot sums double products, four at a time then the tail; cv::pow(.,2) is x*x in float.
* O1 - s*R*O2 is one gemm with alpha = -s, beta = 1; s*R is convertTo(s); (1.0/s)*R.t() is the
  transpose, then convertTo(1.0/s) unless that factor is exactly 1; -sRinv*t is the small gemm with
  alpha = -1.

`counters` records how often the quirk branches fired so a test can assert its input reaches them.
"""
import collections
import math

import numpy as np

F32 = np.float32
F64 = np.float64
RAND_MAX = 2147483647
INT_MIN = -2147483648


# ------------------------------------------------------------------ shared deterministic math (twins)
def atan2_det(y, x):
    """Python twin of orbx_device.h atan2_det (doubles, the same operation sequence)."""
    y, x = float(y), float(x)
    if y != y or x != x:
        return y + x
    ny, nx = math.copysign(1.0, y) < 0, math.copysign(1.0, x) < 0
    ay = -y if ny else y
    ax = -x if nx else x
    sw = ay > ax
    hi, lo = (ay, ax) if sw else (ax, ay)
    if hi == 0.0:
        t = 0.0
    elif lo == hi:
        t = 1.0
    else:
        t = lo / hi
    k = float(round(t * 4.0))
    c = k * 0.25
    base = (0.0, 2.44978663126864143e-01, 4.63647609000806094e-01, 6.43501108793284371e-01,
            7.85398163397448279e-01)[int(k)]
    r = (t - c) / (1.0 + t * c)
    r2 = r * r
    p = 1.0 / 23.0
    p = p * r2 - 1.0 / 21.0
    p = p * r2 + 1.0 / 19.0
    p = p * r2 - 1.0 / 17.0
    p = p * r2 + 1.0 / 15.0
    p = p * r2 - 1.0 / 13.0
    p = p * r2 + 1.0 / 11.0
    p = p * r2 - 1.0 / 9.0
    p = p * r2 + 1.0 / 7.0
    p = p * r2 - 1.0 / 5.0
    p = p * r2 + 1.0 / 3.0
    a = base + (r - r * (r2 * p))
    if sw:
        a = (1.57079632679489656e+00 - a) + 6.12323399573676604e-17
    if nx:
        a = (3.14159265358979312e+00 - a) + 1.22464679914735321e-16
    return -a if ny else a


def sincos_d(x):
    """Python twin of orbx_device.h sincos_d."""
    x = float(x)
    if x != x or math.isinf(x):
        return float("nan"), float("nan")
    kd = float(round(x * 6.36619772367581382433e-01))
    q = int(kd)
    r = (x - kd * 1.57079632673412561417e+00) - kd * 6.07710050650619224932e-11
    r2 = r * r
    ps = 1.0 / 51090942171709440000.0
    ps = ps * r2 - 1.0 / 121645100408832000.0
    ps = ps * r2 + 1.0 / 355687428096000.0
    ps = ps * r2 - 1.0 / 1307674368000.0
    ps = ps * r2 + 1.0 / 6227020800.0
    ps = ps * r2 - 1.0 / 39916800.0
    ps = ps * r2 + 1.0 / 362880.0
    ps = ps * r2 - 1.0 / 5040.0
    ps = ps * r2 + 1.0 / 120.0
    ps = ps * r2 - 1.0 / 6.0
    sr = r + r * (r2 * ps)
    pc = 1.0 / 2432902008176640000.0
    pc = pc * r2 - 1.0 / 6402373705728000.0
    pc = pc * r2 + 1.0 / 20922789888000.0
    pc = pc * r2 - 1.0 / 87178291200.0
    pc = pc * r2 + 1.0 / 479001600.0
    pc = pc * r2 - 1.0 / 3628800.0
    pc = pc * r2 + 1.0 / 40320.0
    pc = pc * r2 - 1.0 / 720.0
    pc = pc * r2 + 1.0 / 24.0
    pc = pc * r2 - 0.5
    cr = 1.0 + r2 * pc
    return ((sr, cr), (cr, -sr), (-sr, -cr), (-cr, sr))[q & 3]


# ------------------------------------------------------------------ OpenCV 3.2 pieces
def _hypot(a, b):
    """hypot of modules/core/src/lapack.cpp, float."""
    a, b = abs(a), abs(b)
    if a > b:
        b = b / a
        return a * np.sqrt(F32(1) + b * b)
    if b > 0:
        a = a / b
        return b * np.sqrt(F32(1) + a * a)
    return F32(0)


def jacobi_eigen(N):
    """cv::eigen(N, eval, evec) for an n x n CV_32F symmetric N: JacobiImpl_<float>.  Returns
    (eigenvalues descending, eigenvectors as rows, rotations run)."""
    n = len(N)
    eps = F32(1.1920928955078125e-07)
    A = [[F32(v) for v in row] for row in N]
    V = [[F32(1) if i == j else F32(0) for j in range(n)] for i in range(n)]
    W = [F32(0)] * n
    indR, indC = [0] * n, [0] * n
    for k in range(n):
        W[k] = A[k][k]
        if k < n - 1:
            m, mv = k + 1, abs(A[k][k + 1])
            for i in range(k + 2, n):
                val = abs(A[k][i])
                if mv < val:
                    mv, m = val, i
            indR[k] = m
        if k > 0:
            m, mv = 0, abs(A[0][k])
            for i in range(1, k):
                val = abs(A[i][k])
                if mv < val:
                    mv, m = val, i
            indC[k] = m
    rotations = 0
    for _ in range(n * n * 30):
        k, mv = 0, abs(A[0][indR[0]])
        for i in range(1, n - 1):
            val = abs(A[i][indR[i]])
            if mv < val:
                mv, k = val, i
        l = indR[k]
        for i in range(1, n):
            val = abs(A[indC[i]][i])
            if mv < val:
                mv, k, l = val, indC[i], i
        p = A[k][l]
        if abs(p) <= eps:
            break
        rotations += 1
        y = F32(F64(W[l] - W[k]) * F64(0.5))
        t = abs(y) + _hypot(p, y)
        s = _hypot(p, t)
        c = t / s
        s = p / s
        t = (p / t) * p
        if y < 0:
            s, t = -s, -t
        A[k][l] = F32(0)
        W[k] = W[k] - t
        W[l] = W[l] + t

        def rot(a0, b0):
            return a0 * c - b0 * s, a0 * s + b0 * c
        for i in range(0, k):
            A[i][k], A[i][l] = rot(A[i][k], A[i][l])
        for i in range(k + 1, l):
            A[k][i], A[i][l] = rot(A[k][i], A[i][l])
        for i in range(l + 1, n):
            A[k][i], A[l][i] = rot(A[k][i], A[l][i])
        for i in range(n):
            V[k][i], V[l][i] = rot(V[k][i], V[l][i])
        for idx in (k, l):
            if idx < n - 1:
                m, mv = idx + 1, abs(A[idx][idx + 1])
                for i in range(idx + 2, n):
                    val = abs(A[idx][i])
                    if mv < val:
                        mv, m = val, i
                indR[idx] = m
            if idx > 0:
                m, mv = 0, abs(A[0][idx])
                for i in range(1, idx):
                    val = abs(A[i][idx])
                    if mv < val:
                        mv, m = val, i
                indC[idx] = m
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            V[m], V[k] = V[k], V[m]
    return W, V, rotations


def rodrigues(vec, sincos=sincos_d):
    """cv::Rodrigues of a CV_32F rotation vector -> 3x3 CV_32F (row-major list of 9)."""
    rx, ry, rz = F64(vec[0]), F64(vec[1]), F64(vec[2])
    theta = np.sqrt(rx * rx + ry * ry + rz * rz)
    if theta < F64(2.2204460492503131e-16):
        return [F32(1) if k % 4 == 0 else F32(0) for k in range(9)]
    s, c = sincos(theta)
    s, c = F64(s), F64(c)
    c1 = F64(1) - c
    itheta = F64(1) / theta if theta != 0 else F64(0)
    rx, ry, rz = rx * itheta, ry * itheta, rz * itheta
    rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
    r_x = [F64(0), -rz, ry, rz, F64(0), -rx, -ry, rx, F64(0)]
    return [F32(c * F64(1 if k % 4 == 0 else 0) + c1 * rrt[k] + s * r_x[k]) for k in range(9)]


def _centroid(P):
    """ComputeCentroid (:247-262); P 3x3 (rows x, y, z; one point per column) -> (Pr, C)."""
    third = F32(1.0 / 3.0)
    Pr, C = [], []
    for r in range(3):
        s = (P[r][0] + P[r][2]) + P[r][1]
        c = s * third + F32(0)
        C.append(c)
        Pr.append([P[r][j] - c for j in range(3)])
    return Pr, C


def compute_sim3(P1, P2, fix_scale, atan2=atan2_det, counters=None, sincos=sincos_d):
    """ComputeSim3 (:264-393).  P1, P2: 3x3 float32, one point per column.  Returns a dict with
    R (9), t (3), s, T12 (16), T21 (16) as float32."""
    Pr1, O1 = _centroid(P1)
    Pr2, O2 = _centroid(P2)
    M = [[F32((F64(0) + F64(Pr2[i][0]) * F64(Pr1[j][0]) + F64(Pr2[i][1]) * F64(Pr1[j][1]) +
               F64(Pr2[i][2]) * F64(Pr1[j][2])) * F64(1)) for j in range(3)] for i in range(3)]
    N11 = M[0][0] + M[1][1] + M[2][2]
    N12 = M[1][2] - M[2][1]
    N13 = M[2][0] - M[0][2]
    N14 = M[0][1] - M[1][0]
    N22 = M[0][0] - M[1][1] - M[2][2]
    N23 = M[0][1] + M[1][0]
    N24 = M[2][0] + M[0][2]
    N33 = -M[0][0] + M[1][1] - M[2][2]
    N34 = M[1][2] + M[2][1]
    N44 = -M[0][0] - M[1][1] + M[2][2]
    N = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
    _, evec, _ = jacobi_eigen(N)
    vec = [evec[0][1], evec[0][2], evec[0][3]]
    nrm = np.sqrt(F64(vec[0]) * F64(vec[0]) + F64(vec[1]) * F64(vec[1]) + F64(vec[2]) * F64(vec[2]))
    ang = F64(atan2(float(nrm), float(evec[0][0])))
    if counters is not None:
        if evec[0][0] < 0:
            counters["negative_real_part"] += 1
        if nrm == 0:
            counters["zero_norm"] += 1
    alpha = F32((F64(2) * ang) * (F64(1) / nrm))
    vec = [v * alpha + F32(0) for v in vec]
    R = rodrigues(vec, sincos)
    P3 = [[(R[3 * i] * Pr2[0][j] + R[3 * i + 1] * Pr2[1][j] + R[3 * i + 2] * Pr2[2][j]) + F32(0) for j in range(3)]
          for i in range(3)]
    if not fix_scale:
        a = [Pr1[i][j] for i in range(3) for j in range(3)]
        b = [P3[i][j] for i in range(3) for j in range(3)]
        pr = [F64(a[k]) * F64(b[k]) for k in range(9)]
        nom = F64(0)
        nom = nom + (pr[0] + pr[1] + pr[2] + pr[3])
        nom = nom + (pr[4] + pr[5] + pr[6] + pr[7])
        nom = nom + pr[8]
        den = F64(0)
        for k in range(9):
            den = den + F64(b[k] * b[k])
        s12 = F32(nom / den)
    else:
        s12 = F32(1)
    t12 = []
    for i in range(3):
        t0 = R[3 * i] * O2[0] + R[3 * i + 1] * O2[1] + R[3 * i + 2] * O2[2]
        t12.append(F32(F64(t0) * (-F64(s12)) + F64(O1[i]) * F64(1)))
    sR = [r * s12 + F32(0) for r in R]
    ia = F64(1) / F64(s12)
    if ia != 1:
        iaf = F32(ia)
        sRinv = [R[3 * j + i] * iaf + F32(0) for i in range(3) for j in range(3)]
    else:
        sRinv = [R[3 * j + i] for i in range(3) for j in range(3)]
    tinv = []
    for i in range(3):
        t0 = sRinv[3 * i] * t12[0] + sRinv[3 * i + 1] * t12[1] + sRinv[3 * i + 2] * t12[2]
        tinv.append(F32(F64(t0) * F64(-1) + F64(0)))
    T12 = np.eye(4, dtype=F32)
    T21 = np.eye(4, dtype=F32)
    for r in range(3):
        for c in range(3):
            T12[r, c] = sR[3 * r + c]
            T21[r, c] = sRinv[3 * r + c]
        T12[r, 3] = t12[r]
        T21[r, 3] = tinv[r]
    return {"R": np.array(R, F32).reshape(3, 3), "t": np.array(t12, F32), "s": F32(s12), "T12": T12, "T21": T21}


def project(X, T, K):
    """Project (:440-461): X [n,3] float32 through T (4x4) with K = (fx, fy, cx, cy) -> [n,2]."""
    X = np.asarray(X, F32).reshape(-1, 3)
    P = []
    for r in range(3):
        t0 = T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1] + T[r, 2] * X[:, 2]
        P.append((t0.astype(F64) * F64(1) + F64(T[r, 3]) * F64(1)).astype(F32))
    return _pinhole(P[0], P[1], P[2], K)


def _pinhole(X, Y, Z, K):
    fx, fy, cx, cy = (F32(v) for v in K)
    invz = F32(1) / Z
    x = X * invz
    y = Y * invz
    return np.stack([fx * x + cx, fy * y + cy], axis=1).astype(F32)


def from_camera_to_image(X, K):
    """FromCameraToImage (:463-481)."""
    X = np.asarray(X, F32).reshape(-1, 3)
    return _pinhole(X[:, 0], X[:, 1], X[:, 2], K)


def max_error(sigma2):
    """mvnMaxError (:95-96, include/Sim3Solver.h:87-88): 9.210 * sigma2 in double, truncated to
    size_t; compared against a float error it converts to float."""
    return np.array([F32(int(F64(9.210) * F64(F32(s)))) for s in np.asarray(sigma2).reshape(-1)], F32)


def ransac_iterations(N, probability, min_inliers, max_iterations):
    """mRansacMaxIts of SetRansacParameters (:127-151)."""
    with np.errstate(all="ignore"):
        epsilon = F32(min_inliers) / F32(N)
        if min_inliers == N:
            n_it = 1
        else:
            e3 = math.pow(float(epsilon), 3.0) if np.isfinite(epsilon) else float(epsilon)
            a, b = 1.0 - float(probability), 1.0 - e3
            num = math.log(a) if a > 0 else (float("-inf") if a == 0 else float("nan"))
            den = math.log(b) if b > 0 else (float("-inf") if b == 0 else float("nan"))
            v = float(np.ceil(F64(num) / F64(den)))
            # the x86 double -> int conversion: NaN and out-of-range give INT_MIN
            n_it = int(v) if (v == v and -2147483649.0 < v < 2147483648.0) else INT_MIN
    return max(1, min(n_it, int(max_iterations)))


class Sim3Solver:
    """The reference class on gathered correspondences (the constructor's loop, :63-115, is the
    caller's; gather() below restates it for an object graph)."""

    def __init__(self, x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2, bFixScale, mvnIndices1=None, mN1=None,
                 atan2=atan2_det):
        self.mvX3Dc1 = np.ascontiguousarray(x3dc1, F32).reshape(-1, 3)
        self.mvX3Dc2 = np.ascontiguousarray(x3dc2, F32).reshape(-1, 3)
        n = len(self.mvX3Dc1)
        self.mvnIndices1 = list(range(n)) if mvnIndices1 is None else [int(i) for i in mvnIndices1]
        self.mN1 = n if mN1 is None else int(mN1)
        self.mK1, self.mK2 = tuple(K1), tuple(K2)
        self.mbFixScale = bool(bFixScale)
        self.atan2 = atan2
        self.counters = collections.Counter()
        with np.errstate(all="ignore"):
            self.mvnMaxError1 = max_error(sigma2_1)
            self.mvnMaxError2 = max_error(sigma2_2)
            self.mvP1im1 = from_camera_to_image(self.mvX3Dc1, self.mK1)
            self.mvP2im2 = from_camera_to_image(self.mvX3Dc2, self.mK2)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.mvbBestInliers = np.zeros(n, bool)
        self.mBestT12 = np.zeros((4, 4), F32)
        self.mBestRotation = np.zeros((3, 3), F32)
        self.mBestTranslation = np.zeros(3, F32)
        self.mBestScale = F32(0)
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self.mRansacProb = probability
        self.mRansacMinInliers = int(minInliers)
        self.N = len(self.mvX3Dc1)
        self.mRansacMaxIts = ransac_iterations(self.N, probability, minInliers, maxIterations)
        self.mnIterations = 0

    def check_inliers(self, H):
        with np.errstate(all="ignore"):
            vP2im1 = project(self.mvX3Dc2, H["T12"], self.mK1)
            vP1im2 = project(self.mvX3Dc1, H["T21"], self.mK2)
            d1 = self.mvP1im1 - vP2im1
            d2 = vP1im2 - self.mvP2im2
            e1 = (d1[:, 0].astype(F64) * d1[:, 0].astype(F64) + d1[:, 1].astype(F64) * d1[:, 1].astype(F64)).astype(F32)
            e2 = (d2[:, 0].astype(F64) * d2[:, 0].astype(F64) + d2[:, 1].astype(F64) * d2[:, 1].astype(F64)).astype(F32)
            return (e1 < self.mvnMaxError1) & (e2 < self.mvnMaxError2)

    def hypothesis(self, idx):
        """ComputeSim3 of the pairs idx (3 indices)."""
        P1 = [[self.mvX3Dc1[idx[c], r] for c in range(3)] for r in range(3)]
        P2 = [[self.mvX3Dc2[idx[c], r] for c in range(3)] for r in range(3)]
        with np.errstate(all="ignore"):
            return compute_sim3(P1, P2, self.mbFixScale, self.atan2, self.counters)

    def iterate(self, nIterations, rng):
        """iterate (:153-239); rng.rand() is the process rand().  Returns (T12 or None, bNoMore,
        vbInliers[mN1], nInliers)."""
        vbInliers = np.zeros(self.mN1, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, vbInliers, 0
        nCurrent = 0
        while self.mnIterations < self.mRansacMaxIts and nCurrent < nIterations:
            nCurrent += 1
            self.mnIterations += 1
            avail = list(range(self.N))
            idx = []
            for _ in range(3):
                randi = int((float(rng.rand()) / (float(RAND_MAX) + 1.0)) * len(avail))
                idx.append(avail[randi])
                avail[randi] = avail[-1]
                avail.pop()
            H = self.hypothesis(idx)
            inl = self.check_inliers(H)
            n_in = int(inl.sum())
            if self.mRansacMinInliers < n_in < self.mnBestInliers:
                self.counters["good_below_best"] += 1
            if n_in >= self.mnBestInliers:
                self.mvbBestInliers = inl
                self.mnBestInliers = n_in
                self.mBestT12 = H["T12"].copy()
                self.mBestRotation = H["R"].copy()
                self.mBestTranslation = H["t"].copy()
                self.mBestScale = H["s"]
                if n_in > self.mRansacMinInliers:
                    for i in range(self.N):
                        if inl[i]:
                            vbInliers[self.mvnIndices1[i]] = True
                    return self.mBestT12.copy(), False, vbInliers, n_in
                if n_in == 0 and np.isnan(H["T12"]).any():
                    self.counters["nan_best"] += 1
        return None, self.mnIterations >= self.mRansacMaxIts, vbInliers, 0

    def find(self, rng):
        T, _, vb, n = self.iterate(self.mRansacMaxIts, rng)
        return T, vb, n

    def GetEstimatedRotation(self):
        return self.mBestRotation.copy()

    def GetEstimatedTranslation(self):
        return self.mBestTranslation.copy()

    def GetEstimatedScale(self):
        return self.mBestScale


def mat3x1(R, t, X):
    """Rcw*X + tcw on 3x1 CV_32F Mats: cv::gemm(R, X, 1, t, 1), the small-matrix path."""
    out = []
    for r in range(3):
        t0 = F32(R[r][0]) * F32(X[0]) + F32(R[r][1]) * F32(X[1]) + F32(R[r][2]) * F32(X[2])
        out.append(F32(F64(t0) * F64(1) + F64(F32(t[r])) * F64(1)))
    return out


def gather(kf1, kf2, vpMatched12):
    """The constructor's loop (:63-115) over a small object graph.  kfj: dict with Tcw (4x4),
    mappoints (list of None or point dicts), keys_octave (per keypoint), level_sigma2; a point dict
    has pos (3), bad (bool) and index (dict: keyframe id -> index or absent = -1).  vpMatched12:
    list (per keypoint of kf1) of None or point dicts of kf2.  Returns the gathered arrays."""
    T1, T2 = np.asarray(kf1["Tcw"], F32), np.asarray(kf2["Tcw"], F32)
    x1, x2, s1, s2, ind = [], [], [], [], []
    for i1, pMP2 in enumerate(vpMatched12):
        if pMP2 is None:
            continue
        pMP1 = kf1["mappoints"][i1]
        if pMP1 is None:
            continue
        if pMP1["bad"] or pMP2["bad"]:
            continue
        i_kf1 = pMP1["index"].get(kf1["id"], -1)
        i_kf2 = pMP2["index"].get(kf2["id"], -1)
        if i_kf1 < 0 or i_kf2 < 0:
            continue
        s1.append(F32(kf1["level_sigma2"][kf1["keys_octave"][i_kf1]]))
        s2.append(F32(kf2["level_sigma2"][kf2["keys_octave"][i_kf2]]))
        ind.append(i1)
        x1.append(mat3x1(T1[:3, :3], T1[:3, 3], pMP1["pos"]))
        x2.append(mat3x1(T2[:3, :3], T2[:3, 3], pMP2["pos"]))
    return {"x3dc1": np.array(x1, F32).reshape(-1, 3), "x3dc2": np.array(x2, F32).reshape(-1, 3),
            "sigma2_1": np.array(s1, F32), "sigma2_2": np.array(s2, F32), "mvnIndices1": ind,
            "mN1": len(vpMatched12)}

"""A literal Python restatement of the reference's Optimizer::OptimizeSim3 (src/Optimizer.cc:1220-1456)
with the g2o pieces it runs -- the yardstick of tests/test_optsim3.py and tests/test_optsim3_shim.py.
It is not the code under test and needs no GPU.

Every arithmetic step is one IEEE double operation, on a Python float (the Sim3 vertex, the LM state,
the dense solve) or elementwise on numpy float64 arrays over the edges (errors, Jacobian columns,
quadratic-form terms).  The sums g2o forms over the edges run as sequential Python-float chains in edge
insertion order e12_0, e21_0, e12_1, e21_1, ...  Parity against the genuine g2o/Eigen binary is
unpinned, as for PoseOptimization: the evaluation orders below are the ones Eigen 3's
fixed-size expression templates produce when read from their sources, written down so a later pinning
has one place to correct.

Evaluation orders, choice by choice:

* Vector3d::norm() is sqrt((w0*w0 + w1*w1) + w2*w2).
* Omega*Omega and W*upsilon (3x3 products) sum their three products left to right.
* `I + Omega + Omega*Omega` is (I + Omega) + Omega2 per entry; `I + a*Omega + b*Omega2` is
  (I + a*Omega) + b*Omega2 with a = sin/theta and b = (1 - cos)/(theta*theta) formed first;
  `A*Omega + B*Omega2 + C*I` is (A*Omega + B*Omega2) + C*I per entry (the C*0 off the diagonal is kept:
  it turns a -0 into +0).
* `(C-((b-1)*sigma+a*theta)/(c))*1./(theta2)` parses as ((C - X/c) * 1.) / theta2.
* Quaterniond(R) is Eigen's trace / largest-diagonal conversion (poseopt.hip mat2q's operation order) and
  Sim3 never normalises it; q*q' and q*v are poseopt.hip's qmul and qrot (Eigen's product and
  _transformVector: uv = 2 (q.vec x v); v + w uv + q.vec x uv, summed left to right).
* map(): s*(r*xyz) + t per component; inverse(): conj(r), conj(r)*((-1./s)*t), 1./s; operator*: r*r',
  s*(r*t') + t, s*s'.
* project is x/z, y/z; cam_map is v*f + c; the error is obs - that.
* chi2() = e0*(w*e0) + e1*(w*e1) with w the (diagonal) information entry: the products with the
  information matrix's zero off-diagonals are dropped, as the PoseOptimization restatement drops them.
* The robust quadratic form: omega_r_k = (-(w*e_k))*rho1; b_r += J0r*omega_r_0 + J1r*omega_r_1;
  H_rc += (J0r*(rho1*w))*J0c + (J1r*(rho1*w))*J1c (B^T * weightedOmega evaluated first, then * B).
* std::exp(sigma) is exp_det and sin/cos are sincos_d (twins of orbx_device.h), where the reference calls
  the host libm.
* The LM loop, lambda_0 = 1e-5 max|H_jj|, the _nBad rule, "the rejected trial's errors stay in the
  edges" and the skipped update after a !isPositive solve are oracle/poseopt.cpp's restatement of
  optimization_algorithm_levenberg.cpp / sparse_optimizer.cpp / robust_kernel_impl.cpp (Huber's dsqr is
  a float there), at 7 unknowns.  oplusImpl writes update[6] = 0 into the solver's x when _fix_scale, so
  computeScale reads the zeroed entry.

`counters` records how often each branch fired so a test can assert its input reaches them.
"""
import collections
import fractions
import math
import struct

import numpy as np

from sim3_literal import mat3x1, sincos_d  # the shared twins

F32 = np.float32
F64 = np.float64
EPS = 0.00001
DBL_MAX = 1.7976931348623157e308
DBL_MIN = 2.2250738585072014e-308


# ------------------------------------------------------------------ exp_det (twin of orbx_device.h)
def exp_det(x):
    """Python twin of orbx_device.h exp_det: e^x from basic IEEE operations only.

    k = rint(x/ln2); r = (x - k*ln2_hi) - k*ln2_lo (Cody-Waite: ln2_hi has 21 trailing zero bits, so
    k*ln2_hi is exact for |k| < 2^11); p = sum_{j=2..13} r^(j-2)/j! by Horner; e^r = 1 + (r + (r*r)*p);
    the result is that times 2^k, exact (k is clamped to the normal exponents, so the supported domain is
    |x| <= 708).  At x = 0: k = 0, r = 0 and the result is 1 + (0 + 0*p) = exactly 1.0.

    Error against the true exponential for |x| <= 2, with u = 2^-53 (|k| <= 3, |r| < 0.3466, so e^r lies
    in [0.7071, 1.4143]; the scaling by 2^k is exact, so errors relative to e^r are errors relative to e^x):
      reduction      k*ln2_hi is exact; x - k*ln2_hi is exact (k = 0, or Sterbenz: the two are within a
                     factor 2); subtracting k*ln2_lo rounds once below 0.5, |dr| <= 2^-55 = 0.25 u (ln2_hi +
                     ln2_lo misses ln 2 by < 2^-102, k*ln2_lo rounds below 2^-84: negligible).  e^(r + dr)
                     = e^r (1 + dr): 0.25 u relative, counted as 0.5 u
      truncation     r^14/14! * e^|r| < 0.3466^14 / 14! * 1.42 < 5.9e-18 = 0.053 u, absolute
      Horner         |p| < 0.6 throughout; a step p*r + c rounds the product (<= u * 0.6 * 0.3466), the sum
                     (<= u * 0.6) and carries c's own rounding (<= u * 0.5), and passes the earlier error on
                     times |r|: at most (0.21 + 0.6 + 0.5) u / (1 - 0.3466) = 2.0 u on p, times r*r < 0.1202:
                     0.24 u, absolute
      r*r, (r*r)*p   half an ulp each below 0.125: 2 * 2^-57 = 0.125 u, absolute
      r + (...)      half an ulp below 0.5: 2^-55 = 0.25 u, absolute
      1 + (...)      the final rounding: half an ulp of the result, at most 1 u relative
    The absolute terms sum to (0.053 + 0.24 + 0.125 + 0.25) u = 0.668 u, at most 0.668 / 0.7071 = 0.945 u
    relative; with the reduction's 0.5 u and the final 1 u: |exp_det(x) - e^x| <= 2.5 u e^x = EXP_DET_BOUND.
    """
    x = float(x)
    if x != x:
        return x
    kd = float(round(x * 1.44269504088896338700e+00))
    if kd > 1023.0:
        kd = 1023.0
    if kd < -1022.0:
        kd = -1022.0
    r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10
    p = 1.0 / 6227020800.0
    p = p * r + 1.0 / 479001600.0
    p = p * r + 1.0 / 39916800.0
    p = p * r + 1.0 / 3628800.0
    p = p * r + 1.0 / 362880.0
    p = p * r + 1.0 / 40320.0
    p = p * r + 1.0 / 5040.0
    p = p * r + 1.0 / 720.0
    p = p * r + 1.0 / 120.0
    p = p * r + 1.0 / 24.0
    p = p * r + 1.0 / 6.0
    p = p * r + 0.5
    e = 1.0 + (r + (r * r) * p)
    scale = struct.unpack("<d", struct.pack("<q", (int(kd) + 1023) << 52))[0]
    return e * scale


EXP_DET_BOUND = 2.5 * 2.0 ** -53  # relative, |x| <= 2 (derived in exp_det's docstring)


# ------------------------------------------------------------------ quaternion pieces (poseopt.hip:45-114)
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    w = aw * bw - (ax * bx + ay * by + az * bz)
    x = aw * bx + bw * ax + (ay * bz - az * by)
    y = aw * by + bw * ay + (az * bx - ax * bz)
    z = aw * bz + bw * az + (ax * by - ay * bx)
    return (x, y, z, w)


def qrot(q, v):
    """q scalars; v a triple of floats or of arrays (the same single operations elementwise)."""
    qx, qy, qz, qw = q
    uv = [qy * v[2] - qz * v[1], qz * v[0] - qx * v[2], qx * v[1] - qy * v[0]]
    uv = [u + u for u in uv]
    c = [qy * uv[2] - qz * uv[1], qz * uv[0] - qx * uv[2], qx * uv[1] - qy * uv[0]]
    return [v[i] + qw * uv[i] + c[i] for i in range(3)]


def mat2q(m):
    """Quaterniond(Matrix3d), m row-major list of 9 -> (x, y, z, w); not normalised."""
    t = m[0] + m[4] + m[8]
    if t > 0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return ((m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t, w)
    i = 0
    if m[4] > m[0]:
        i = 1
    if m[8] > (m[0] if i == 0 else m[4]):
        i = 2
    if i == 0:
        t = math.sqrt(m[0] - m[4] - m[8] + 1.0)
        ci = 0.5 * t
        t = 0.5 / t
        return (ci, (m[3] + m[1]) * t, (m[6] + m[2]) * t, (m[7] - m[5]) * t)
    if i == 1:
        t = math.sqrt(m[4] - m[8] - m[0] + 1.0)
        ci = 0.5 * t
        t = 0.5 / t
        return ((m[1] + m[3]) * t, ci, (m[7] + m[5]) * t, (m[2] - m[6]) * t)
    t = math.sqrt(m[8] - m[0] - m[4] + 1.0)
    ci = 0.5 * t
    t = 0.5 / t
    return ((m[2] + m[6]) * t, (m[5] + m[7]) * t, ci, (m[3] - m[1]) * t)


# ------------------------------------------------------------------ g2o::Sim3 (types/sim3.h:41-292)
# a Sim3 is (q, t, s) with q = (x, y, z, w), t a list of 3; as eight doubles: q, t, s.
def sim3_from8(v):
    v = [float(a) for a in v]
    return ((v[0], v[1], v[2], v[3]), [v[4], v[5], v[6]], v[7])


def sim3_to8(S):
    return np.array(list(S[0]) + list(S[1]) + [S[2]], F64)


BRANCHES = ("small_sigma_small_theta", "small_sigma_theta", "sigma_small_theta", "sigma_theta")


def sim3_exp(update, counters=None):
    """Sim3(const Vector7d&), sim3.h:70-142."""
    w = [float(update[0]), float(update[1]), float(update[2])]
    up = [float(update[3]), float(update[4]), float(update[5])]
    sigma = float(update[6])
    theta = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    O = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    s = exp_det(sigma)
    O2 = [O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c] + O[3 * r + 2] * O[6 + c] for r in range(3) for c in range(3)]
    I = [1.0 if k % 4 == 0 else 0.0 for k in range(9)]
    if abs(sigma) < EPS:
        C = 1.0
        if theta < EPS:
            branch = 0
            A = 1. / 2.
            B = 1. / 6.
            R = [I[k] + O[k] + O2[k] for k in range(9)]
        else:
            branch = 1
            sn, cs = sincos_d(theta)
            theta2 = theta * theta
            A = (1 - cs) / theta2
            B = (theta - sn) / (theta2 * theta)
            a, b = sn / theta, (1 - cs) / (theta * theta)
            R = [I[k] + a * O[k] + b * O2[k] for k in range(9)]
    else:
        C = (s - 1) / sigma
        if theta < EPS:
            branch = 2
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            R = [I[k] + O[k] + O2[k] for k in range(9)]
        else:
            branch = 3
            sn, cs = sincos_d(theta)
            a, b = sn / theta, (1 - cs) / (theta * theta)
            R = [I[k] + a * O[k] + b * O2[k] for k in range(9)]
            a = s * sn
            b = s * cs
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    if counters is not None:
        counters["exp_" + BRANCHES[branch]] += 1
    q = mat2q(R)
    W = [A * O[k] + B * O2[k] + C * I[k] for k in range(9)]
    t = [W[3 * r] * up[0] + W[3 * r + 1] * up[1] + W[3 * r + 2] * up[2] for r in range(3)]
    return (q, t, s)


def sim3_mul(a, b):
    """operator*, sim3.h:266-272."""
    rt = qrot(a[0], b[1])
    return (qmul(a[0], b[0]), [a[2] * rt[i] + a[1][i] for i in range(3)], a[2] * b[2])


def sim3_inverse(S):
    """inverse(), sim3.h:233-236."""
    q, t, s = S
    qc = (-q[0], -q[1], -q[2], q[3])
    c = -1. / s
    return (qc, qrot(qc, [c * t[0], c * t[1], c * t[2]]), 1. / s)


def sim3_map(S, X):
    """map(), sim3.h:144-146; X a triple of floats or arrays."""
    r = qrot(S[0], X)
    return [S[2] * r[i] + S[1][i] for i in range(3)]


def oplus(S, update, fix_scale, counters=None):
    """VertexSim3Expmap::oplusImpl: update[6] is zeroed IN PLACE when _fix_scale."""
    if fix_scale:
        update[6] = 0.0
    return sim3_mul(sim3_exp(update, counters), S)


# ------------------------------------------------------------------ the two edges
def error12(S, X2, obs, K):
    """EdgeSim3ProjectXYZ::computeError (:138-153): obs1 - cam_map1(project(S.map(X2)))."""
    p = sim3_map(S, X2)
    return obs[0] - (p[0] / p[2] * K[0] + K[2]), obs[1] - (p[1] / p[2] * K[1] + K[3])


def error21(S, X1, obs, K):
    """EdgeInverseSim3ProjectXYZ::computeError (:168-183): obs2 - cam_map2(project(S.inverse().map(X1)))."""
    p = sim3_map(sim3_inverse(S), X1)
    return obs[0] - (p[0] / p[2] * K[0] + K[2]), obs[1] - (p[1] / p[2] * K[1] + K[3])


DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)


def numeric_jacobian(S, fix_scale, err):
    """BaseBinaryEdge::linearizeOplus, the Sim3 side (base_binary_edge.hpp:147-200): err(S) -> (e0, e1).
    Returns (J0[7], J1[7]), the rows of the 2x7 _jacobianOplusXj."""
    J0, J1 = [], []
    for d in range(7):
        add = [0.0] * 7
        add[d] = DELTA
        ep = err(oplus(S, add, fix_scale))
        add[d] = -DELTA
        em = err(oplus(S, add, fix_scale))
        J0.append(SCALAR * (ep[0] - em[0]))
        J1.append(SCALAR * (ep[1] - em[1]))
    return J0, J1


# ------------------------------------------------------------------ Eigen::LDLT<MatrixXd> + isPositive()
def ldlt_solve(Hin, b, n):
    """oracle/poseopt.cpp ldlt6 (:306-370) at n unknowns.  Hin row-major n*n, b n -> (ok, x)."""
    m = [float(v) for v in Hin]
    tr = list(range(n))
    sign = 0
    for k in range(n):
        big, bv = k, abs(m[(n + 1) * k])
        for i in range(k + 1, n):
            if abs(m[(n + 1) * i]) > bv:
                bv, big = abs(m[(n + 1) * i]), i
        if k == 0 and not (bv > 0.0):
            tr = list(range(n))
            for j in range(n):
                m[(n + 1) * j] = 0.0
            sign = 0
            break
        tr[k] = big
        if k != big:
            for j in range(k):
                m[n * k + j], m[n * big + j] = m[n * big + j], m[n * k + j]
            for i in range(big + 1, n):
                m[n * i + k], m[n * i + big] = m[n * i + big], m[n * i + k]
            m[(n + 1) * k], m[(n + 1) * big] = m[(n + 1) * big], m[(n + 1) * k]
            for i in range(k + 1, big):
                m[n * i + k], m[n * big + i] = m[n * big + i], m[n * i + k]
        if k > 0:
            temp = [m[(n + 1) * j] * m[n * k + j] for j in range(k)]
            dot = m[n * k] * temp[0]
            for j in range(1, k):
                dot = dot + m[n * k + j] * temp[j]
            m[(n + 1) * k] -= dot
            for i in range(k + 1, n):
                s = m[n * i] * temp[0]
                for j in range(1, k):
                    s = s + m[n * i + j] * temp[j]
                m[n * i + k] -= s
        akk = m[(n + 1) * k]
        if abs(akk) > 0.0:
            for i in range(k + 1, n):
                m[n * i + k] /= akk
        if akk > 0:
            sign = 3 if sign in (2, 3) else 1
        elif akk < 0:
            sign = 3 if sign in (1, 3) else 2
    if sign not in (0, 1):
        return False, [0.0] * n
    y = [float(v) for v in b]
    for k in range(n):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    for i in range(n):
        for j in range(i):
            y[i] -= m[n * i + j] * y[j]
    for i in range(n):
        y[i] = y[i] / m[(n + 1) * i] if abs(m[(n + 1) * i]) > DBL_MIN else 0.0
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            y[i] -= m[n * j + i] * y[j]
    for k in range(n - 1, -1, -1):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    return True, y


# ------------------------------------------------------------------ the optimizer
def cube_product(x):
    """t3 * t3 * t3, as oracle/poseopt.cpp writes OptimizationAlgorithmLevenberg's pow(2 rho - 1, 3): the
    cube of PoseOptimization, OptimizeSim3 and OptimizeEssentialGraph."""
    return x * x * x


def cube_rounded(x):
    """x^3 rounded once: LocalBundleAdjustment's cube.  oracle/localba.cpp calls std::pow(x, 3); glibc's pow
    is within an ulp of this value but not always equal to it (x = 6.118015287389873 is one last bit off),
    so the exact rational cube, rounded by float(), is the reference."""
    if not math.isfinite(x):
        return x * x * x
    try:
        return float(fractions.Fraction(x) ** 3)
    except OverflowError:
        return math.copysign(math.inf, x)


def lm_trial(state, tempChi, scale, ok2, cube=cube_product, counters=None):
    """One trial's verdict of OptimizationAlgorithmLevenberg::solve (oracle/poseopt.cpp:441-466), pure.
    state = (lam, ni, currentChi, rho, qmax, nBad); scale = sum x_j (lam x_j + b_j) of a successful solve.
    Returns (state, accepted, another trial follows).  counters (optional): the branch taken."""
    lam, ni, currentChi, rho, qmax, nBad = state
    c = collections.Counter() if counters is None else counters
    if not ok2:
        tempChi = DBL_MAX
        scale = 0.0
        c["not_ok2"] += 1
    rho = currentChi - tempChi
    scale += 1e-3
    rho /= scale
    accept = rho > 0 and math.isfinite(tempChi)
    if accept:
        t3 = 2 * rho - 1
        alpha = 1. - cube(t3)
        c["alpha_above_2/3" if alpha > 2. / 3. else "alpha_below_1/3" if alpha < 1. / 3. else "alpha_between"] += 1
        alpha = min(alpha, 2. / 3.)
        lam *= max(1. / 3., alpha)
        ni = 2.0
        currentChi = tempChi
    else:
        c["reject_rho_nan" if rho != rho else "reject_rho_le_0" if rho <= 0 else "reject_nonfinite_chi"] += 1
        lam *= ni
        ni *= 2
    qmax += 1
    go = rho < 0 and qmax < 10
    if rho < 0 and not go:
        c["tenth_trial"] += 1
    return (lam, ni, currentChi, rho, qmax, nBad), accept, go


def lm_iteration_end(state, iniChi, counters=None):
    """The rule after an iteration's last trial (oracle/poseopt.cpp:467-471 and optimize()'s _nBad
    count), pure.  Returns (state, optimize() stops)."""
    lam, ni, currentChi, rho, qmax, nBad = state
    c = collections.Counter() if counters is None else counters
    if qmax == 10 or rho == 0:
        c["stop_qmax_10" if qmax == 10 else "stop_rho_0"] += 1
        return state, True
    if (iniChi - currentChi) * 1e3 < iniChi:
        nBad += 1
        c["nbad_up"] += 1
    else:
        nBad = 0
        c["nbad_reset"] += 1
    if nBad >= 3:
        c["stop_nbad_3"] += 1
    return (lam, ni, currentChi, rho, qmax, nBad), nBad >= 3


class _Graph:
    """The one-vertex graph after the intake loop, with g2o's Levenberg over it."""

    def __init__(self, P, counters):
        self.X1 = np.ascontiguousarray(P["x3dc1"], F32).reshape(-1, 3).astype(F64)
        self.X2 = np.ascontiguousarray(P["x3dc2"], F32).reshape(-1, 3).astype(F64)
        self.o1 = np.ascontiguousarray(P["obs1"], F32).reshape(-1, 2).astype(F64)
        self.o2 = np.ascontiguousarray(P["obs2"], F32).reshape(-1, 2).astype(F64)
        self.w1 = np.ascontiguousarray(P["inv_sigma2_1"], F32).reshape(-1).astype(F64)
        self.w2 = np.ascontiguousarray(P["inv_sigma2_2"], F32).reshape(-1).astype(F64)
        self.K1 = [float(F32(v)) for v in P["K1"]]
        self.K2 = [float(F32(v)) for v in P["K2"]]
        self.fix = bool(P["bFixScale"])
        self.delta = float(np.sqrt(F32(P["th2"])))  # const float deltaHuber = sqrt(th2)
        self.dsqr = float(F32(self.delta * self.delta))  # RobustKernelHuber::dsqr is a float
        self.S = sim3_from8(P["S12"])
        n = len(self.X1)
        self.E12 = np.zeros((n, 2))
        self.E21 = np.zeros((n, 2))
        self.act = np.arange(n)
        self.counters = counters
        self.trials = 0
        self.lam, self.ni, self.nBad = 0.0, 2.0, 0
        self.last_rejected = False

    def _cols(self, A, idx):
        return [A[idx, k] for k in range(A.shape[1])]

    def errors(self):  # computeActiveErrors
        a = self.act
        e = error12(self.S, self._cols(self.X2, a), self._cols(self.o1, a), self.K1)
        self.E12[a, 0], self.E12[a, 1] = e
        e = error21(self.S, self._cols(self.X1, a), self._cols(self.o2, a), self.K2)
        self.E21[a, 0], self.E21[a, 1] = e

    def edge_chi2(self, E, w, a):
        return E[a, 0] * (w[a] * E[a, 0]) + E[a, 1] * (w[a] * E[a, 1])

    def huber(self, chi):
        """RobustKernelHuber::robustify, rho[0] and rho[1] (oracle/poseopt.cpp:241-252)."""
        with np.errstate(all="ignore"):
            sq = np.sqrt(chi)
            inl = chi <= self.dsqr
            return np.where(inl, chi, 2 * sq * self.delta - self.dsqr), np.where(inl, 1., self.delta / sq)

    def chi2(self):  # activeRobustChi2
        a = self.act
        r12, _ = self.huber(self.edge_chi2(self.E12, self.w1, a))
        r21, _ = self.huber(self.edge_chi2(self.E21, self.w2, a))
        s = 0.0
        for u, v in zip(r12.tolist(), r21.tolist()):
            s = s + u
            s = s + v
        return s

    def _terms(self, E, w, J0, J1):
        """constructQuadraticForm's robust branch for one edge type over the active pairs: 28 H (upper,
        row-major) + 7 b term arrays."""
        chi = E[:, 0] * (w * E[:, 0]) + E[:, 1] * (w * E[:, 1])
        _, rho1 = self.huber(chi)
        wo = rho1 * w
        om0 = (-(w * E[:, 0])) * rho1
        om1 = (-(w * E[:, 1])) * rho1
        out = []
        for r in range(7):
            for c in range(r, 7):
                out.append((J0[r] * wo) * J0[c] + (J1[r] * wo) * J1[c])
        for r in range(7):
            out.append(J0[r] * om0 + J1[r] * om1)
        return [np.broadcast_to(t, chi.shape).tolist() for t in out]

    def build(self):  # linearizeOplus + constructQuadraticForm of every active edge, in order
        a = self.act
        X1, X2, o1, o2 = self._cols(self.X1, a), self._cols(self.X2, a), self._cols(self.o1, a), self._cols(self.o2, a)
        Ja = numeric_jacobian(self.S, self.fix, lambda S: error12(S, X2, o1, self.K1))
        Jb = numeric_jacobian(self.S, self.fix, lambda S: error21(S, X1, o2, self.K2))
        ta = self._terms(self.E12[a], self.w1[a], *Ja)
        tb = self._terms(self.E21[a], self.w2[a], *Jb)
        acc = []
        for k in range(35):
            s = 0.0
            for u, v in zip(ta[k], tb[k]):
                s = s + u
                s = s + v
            acc.append(s)
        H = [0.0] * 49
        k = 0
        for r in range(7):
            for c in range(r, 7):
                H[7 * r + c] = H[7 * c + r] = acc[k]
                k += 1
        self.H, self.b = H, acc[28:35]

    def iteration(self, it):  # OptimizationAlgorithmLevenberg::solve (oracle/poseopt.cpp:421-471)
        self.errors()
        currentChi = self.chi2()
        iniChi = currentChi
        self.build()
        if it == 0:
            m = 0.0
            for j in range(7):
                m = max(abs(self.H[8 * j]), m)
            self.lam, self.ni, self.nBad = 1e-5 * m, 2.0, 0
        rho, qmax = 0.0, 0
        while True:
            bak = self.S
            Hd = list(self.H)
            for j in range(7):
                Hd[8 * j] += self.lam
            ok2, x = ldlt_solve(Hd, self.b, 7)
            self.trials += 1
            if ok2:
                self.S = oplus(self.S, x, self.fix, self.counters)
            else:
                self.counters["not_positive"] += 1
            self.errors()
            tempChi = self.chi2()
            scale = 0.0
            if ok2:
                for j in range(7):
                    scale += x[j] * (self.lam * x[j] + self.b[j])
            (self.lam, self.ni, currentChi, rho, qmax, self.nBad), accept, go = lm_trial(
                (self.lam, self.ni, currentChi, rho, qmax, self.nBad), tempChi, scale, ok2)
            self.last_rejected = not accept
            if not accept:
                self.S = bak  # pop; the rejected trial's errors stay in the edges
                self.counters["rejected_trials"] += 1
            if not go:
                break
        (self.lam, self.ni, currentChi, rho, qmax, self.nBad), stop = lm_iteration_end(
            (self.lam, self.ni, currentChi, rho, qmax, self.nBad), iniChi)
        return not stop

    def optimize(self, its):
        if len(self.act) == 0:
            return 0
        n = 0
        for i in range(its):
            n += 1
            if not self.iteration(i):
                break
        return n

    def bad_pairs(self, th2):
        """e12->chi2() > th2 || e21->chi2() > th2 on the STORED errors (:1402, :1441)."""
        a = self.act
        th = float(F32(th2))
        return (self.edge_chi2(self.E12, self.w1, a) > th) | (self.edge_chi2(self.E21, self.w2, a) > th)


def optimize_sim3(P, counters=None):
    """Optimizer::OptimizeSim3 on gathered correspondences.  P: dict(x3dc1[n,3], x3dc2[n,3], obs1[n,2],
    obs2[n,2], inv_sigma2_1[n], inv_sigma2_2[n], K1, K2 (fx, fy, cx, cy), S12 (8 doubles: quaternion x, y,
    z, w, t, s), th2, bFixScale).  Returns dict(n_in (the return value), S12 (8 doubles; the input when
    the reference does not write g2oS12 back), inlier[n] uint8 (0 where vpMatches1 is nulled), n_bad,
    iterations (2), trials, counters)."""
    counters = collections.Counter() if counters is None else counters
    G = _Graph(P, counters)
    n = len(G.X1)
    S_in = np.array([float(v) for v in P["S12"]], F64)
    inlier = np.ones(n, np.uint8)
    out = {"n_in": 0, "S12": S_in.copy(), "inlier": inlier, "n_bad": 0, "iterations": [0, 0], "trials": 0,
           "counters": counters}
    with np.errstate(all="ignore"):
        out["iterations"][0] = G.optimize(5)
        if G.last_rejected:
            counters["stale_error_pass"] += 1
        bad = G.bad_pairs(P["th2"])
        inlier[G.act[bad]] = 0
        G.act = G.act[~bad]
        nBad = int(bad.sum())
        out["n_bad"] = nBad
        nMore = 10 if nBad > 0 else 5
        counters["nMore_%d" % nMore] += 1
        if n - nBad < 10:
            counters["early_return"] += 1
            out["trials"] = G.trials
            return out
        G.last_rejected = False
        out["iterations"][1] = G.optimize(nMore)
        bad = G.bad_pairs(P["th2"])
        inlier[G.act[bad]] = 0
        out["n_in"] = int((~bad).sum())
        out["S12"] = sim3_to8(G.S)
        out["trials"] = G.trials
    return out


# ------------------------------------------------------------------ the caller's side
def sim3_from_rts(R, t, s):
    """g2o::Sim3(const Matrix3d&, const Vector3d&, double) (sim3.h:64-67) -> 8 doubles."""
    R = np.asarray(R, F64).reshape(9)
    return np.array(list(mat2q([float(v) for v in R])) + [float(v) for v in np.asarray(t, F64).reshape(3)] + [float(s)],
                    F64)


def gather(kf1, kf2, vpMatches1):
    """The intake loop (:1267-1384) over the object graph of sim3_literal.gather, plus per keyframe
    keys_un ([n,2] float32), inv_level_sigma2 and K.  Returns (problem arrays, vnIndexEdge)."""
    T1, T2 = np.asarray(kf1["Tcw"], F32), np.asarray(kf2["Tcw"], F32)
    x1, x2, o1, o2, s1, s2, ind = [], [], [], [], [], [], []
    for i, pMP2 in enumerate(vpMatches1):
        if pMP2 is None:
            continue
        pMP1 = kf1["mappoints"][i]
        i2 = pMP2["index"].get(kf2["id"], -1)
        if pMP1 is None:
            continue
        if pMP1["bad"] or pMP2["bad"] or i2 < 0:
            continue
        x1.append(mat3x1(T1[:3, :3], T1[:3, 3], pMP1["pos"]))
        x2.append(mat3x1(T2[:3, :3], T2[:3, 3], pMP2["pos"]))
        o1.append(kf1["keys_un"][i])
        s1.append(F32(kf1["inv_level_sigma2"][kf1["keys_octave"][i]]))
        o2.append(kf2["keys_un"][i2])
        s2.append(F32(kf2["inv_level_sigma2"][kf2["keys_octave"][i2]]))
        ind.append(i)
    return ({"x3dc1": np.array(x1, F32).reshape(-1, 3), "x3dc2": np.array(x2, F32).reshape(-1, 3),
             "obs1": np.array(o1, F32).reshape(-1, 2), "obs2": np.array(o2, F32).reshape(-1, 2),
             "inv_sigma2_1": np.array(s1, F32), "inv_sigma2_2": np.array(s2, F32), "K1": kf1["K"], "K2": kf2["K"]},
            ind)

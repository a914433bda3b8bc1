"""A literal Python restatement of the reference's Optimizer::PoseOptimization (src/Optimizer.cc:287-528)
with the g2o pieces it runs -- the second yardstick of tests/test_poseopt.py, next to oracle/poseopt.cpp.
It is not the code under test and needs no GPU.

Every arithmetic step is one IEEE double operation, on a Python float (the SE3 vertex, the LM state, the
dense solve) or elementwise on numpy float64 arrays over the edges (errors, Jacobian rows, quadratic-form
terms).  The sums g2o forms over the edges run as sequential Python-float chains in edge insertion order
(functools.reduce over a list of Python floats: s = s + v, one addition per edge).  Parity against the
genuine g2o/Eigen binary is unpinned; the choices below are written down once so a later
pinning has one place to correct.  "reference": read from the reference's sources at the place named.
"oracle": the body is not in the reference tree and the reading of oracle/poseopt.cpp is taken.

The schedule (reference, src/Optimizer.cc)
* :324-325 `const float deltaMono = sqrt(5.991)`: a double square root rounded to float.  The oracle and
  the kernel write sqrtf(5.991f); the two are the same float for 5.991 and for 7.815
  (test_huber_deltas_agree), so no side is wrong.
* :341 mvuRight < 0 makes a monocular edge; :357/:401 the information is the float invSigma2 widened,
  times the identity; :374-376 Xw are floats widened.
* :430 fewer than 3 edges: return 0, the pose untouched.
* :443-518 four rounds.  Each sets the vertex to toSE3Quat(mTcw) (:447), runs optimize(10) on the level-0
  edges, then classifies EVERY edge: an edge flagged an outlier is recomputed at the round's final pose
  (:460-463, :491-494); any other edge keeps the error its last computeError left -- the last TRIAL's, even
  a rejected one, since g2o pops the vertex but not the edges' errors.  `const float chi2 = e->chi2()`
  is compared with the float threshold (:465-467, :496-499).  After the third round the robust kernels
  are dropped (:479, :511).  With fewer than 10 edges only one round runs (:516).
* The mono edges are classified before the stereo ones; an edge's verdict depends on nothing but its own
  error, so the order leaves no trace and the literal walks the edges once.
* :527 the return value is the edge count minus the last round's nBad.

Converter and SE3Quat (reference)
* Converter::toSE3Quat (src/Converter.cc:37-47): R and t from floats widened; SE3Quat(R, t) is
  Quaterniond(R) then normalizeRotation (se3quat.h:58-60).
* normalizeRotation (se3quat.h:280-285): if w < 0 the coefficients are negated; then _r.normalize().
* operator* (se3quat.h:104-110): t = t + r * t2; r = r * r2; normalizeRotation.
* map (se3quat.h:217-220): r * xyz + t.
* exp (se3quat.h:223-257): theta = omega.norm(); theta < 0.00001 takes R = I + Omega + Omega*Omega and
  V = R; else R = I + sin/theta Omega + (1-cos)/(theta*theta) Omega2 and V = I + (1-cos)/(theta*theta) Omega
  + (theta-sin)/pow(theta,3) Omega2; SE3Quat(Quaterniond(R), V*upsilon) normalises.
* Converter::toCvMat(SE3Quat) (src/Converter.cc:49-53): to_homogeneous_matrix, each entry cast to float.

The edges (reference for the declarations, oracle for the bodies)
* computeError (types_six_dof_expmap.h:153-157, :184-188): obs - cam_project(estimate.map(Xw)).
* cam_project and linearizeOplus live in types_six_dof_expmap.cpp, absent from the reference tree -- oracle:
  mono u = x/z*fx + cx; stereo invz = (float)(1/z), u = x*invz*fx + cx, ur = u - bf*invz; the Jacobian
  rows are J0 = [x*y*iz2*fx, -(1+(x*x*iz2))*fx, y*iz*fx, -iz*fx, 0, x*iz2*fx], J1 = [(1+y*y*iz2)*fy,
  -x*y*iz2*fy, -x*iz*fy, 0, -iz*fy, y*iz2*fy], J2 = J0 + [-bf*y*iz2, +bf*x*iz2, 0, 0, 0, -bf*iz2] with
  iz = 1/z in double and iz2 = iz*iz, every product left to right.
* chi2() = e0*(w*e0) + e1*(w*e1) [+ e2*(w*e2)] with w the diagonal information entry (oracle: the
  products with the information matrix's zero off-diagonals are dropped).

The quadratic form (reference for the statement, oracle for Eigen's order)
* BaseUnaryEdge::constructQuadraticForm (core/base_unary_edge.hpp:43-72): with a robust kernel
  b -= rho1 * A^T * omega * e and A += A^T * (rho1*omega) * A; without, the same with rho1 absent.
* oracle: H_rc term = (J0r*w)*J0c + (J1r*w)*J1c [+ (J2r*w)*J2c] with w = rho1*info, the 21 entries of the
  upper triangle; b_r term = ((rho1*J0r)*info)*e0 + ((rho1*J1r)*info)*e1 [+ ...], subtracted from b; without
  a kernel rho1 = 1.0 and w = info (1.0*J is exact, so the same expression serves).
* oracle: the sums over the edges start from +0.0 and add one edge's term at a time.

The kernel and the solver (reference for the headers, oracle for the .cpp bodies)
* RobustKernelHuber (core/robust_kernel_impl.h:76-85): `float dsqr`; robust_kernel.h:71-75 `double
  _delta`.  oracle (robust_kernel_impl.cpp): dsqr = (float)(delta*delta); e <= dsqr gives (e, 1, 0), else
  sq = sqrt(e), rho0 = 2*sq*delta - dsqr, rho1 = delta/sq.
* LinearSolverDense (solvers/linear_solver_dense.h:65-112): Eigen::LDLT of the dense H, `if
  (!ldlt.isPositive()) return false`, x = ldlt.solve(b).  oracle: Eigen's LDLT itself (diagonal pivoting,
  sequential dots) is optsim3_literal.ldlt_solve at n = 6, checked against oracle.ldlt6 bit for bit.
* OptimizationAlgorithmLevenberg (optimization_algorithm_levenberg.h for the members; the .cpp is absent):
  oracle, through optsim3_literal.lm_trial / lm_iteration_end: lambda_0 = 1e-5 max|H_jj|, rho = (chi -
  tempChi) / (sum x_j (lambda x_j + b_j) + 1e-3), accept when rho > 0 and tempChi is finite, lambda *=
  max(1/3, min(1 - (2 rho - 1)^3, 2/3)) with the cube a plain product, else lambda *= ni, ni *= 2 and the
  vertex is popped; up to 10 trials while rho < 0; stop on qmax == 10, rho == 0 or three iterations in a
  row that gained less than a thousandth.  A solve that fails isPositive leaves the vertex alone.
* optimize() with no active edge returns without touching the vertex (oracle; sparse_optimizer.cpp).

Eigen orders (oracle, unpinned)
* Vector3d::norm() is sqrt((w0*w0 + w1*w1) + w2*w2); Quaterniond::normalize() divides by
  sqrt(((x*x + y*y) + z*z) + w*w).
* Omega*Omega and V*upsilon sum their three products left to right; I + a*Omega + b*Omega2 is
  (I + a*Omega) + b*Omega2 per entry with a, b, d formed first; pow(theta, 3) is theta*theta*theta.
* Quaterniond(R), q*q', q*v and toRotationMatrix are optsim3_literal's mat2q, qmul, qrot and qmat below.
* sin/cos are sim3_literal.sincos_d where the reference calls the host libm.

Literal against oracle: the two agree bit for bit (pose bits, flags, return value, iterations per round)
on every case of tests/poseopt_scenes.py and on its device batch, so no item above was decided against either
side.  Unpinned items, where the reference text cannot decide and the oracle is followed: everything under
"Eigen orders", the LDLT's dot-product order, the bodies of types_six_dof_expmap.cpp,
robust_kernel_impl.cpp, optimization_algorithm_levenberg.cpp and sparse_optimizer.cpp -- and one item worth
a name: LinearSolverDense copies the vertex's whole 6x6 block (linear_solver_dense.h:84-99) and Eigen's
LDLT reads the lower triangle, whose entry (c, r) `A.transpose() * weightedOmega * A` forms as
(J_c*w)*J_r, while the oracle (and so the literal and the kernel) mirrors the upper triangle's (J_r*w)*J_c
into it.  The two can differ in the last bit; the reference text cannot decide whether Eigen evaluates both
triangles, so the oracle is followed.

`counters` records how often each branch fired so a test can assert its input reaches them; COUNTERS names
the keys a case table must reach.  huber_outer_* count edges in constructQuadraticForm's robustify;
edge_behind_camera counts error evaluations with depth <= 0.
"""
import collections
import functools
import math
import operator

import numpy as np

from sim3_literal import sincos_d  # the shared twins
from optsim3_literal import cube_product, ldlt_solve, lm_iteration_end, lm_trial, mat2q, qmul, qrot

F32 = np.float32
F64 = np.float64

COUNTERS = ("early_lt3", "one_round_lt10", "round_without_active_edge", "trial_rejected",
            "round_ended_on_rejected_trial", "stop_qmax_10", "stop_nbad_3", "stop_rho_0", "ten_iterations",
            "exp_small_theta", "mat2q_trace", "mat2q_diag0", "mat2q_diag1", "mat2q_diag2", "huber_outer_mono",
            "huber_outer_stereo", "outlier_reinstated", "edge_behind_camera", "solve_not_positive")


def huber_deltas():
    """(deltaMono, deltaStereo) as src/Optimizer.cc:324-325 computes them, as Python floats."""
    return float(F32(math.sqrt(5.991))), float(F32(math.sqrt(7.815)))


# ------------------------------------------------------------------ SE3Quat; a pose is (q, t), q = (x, y, z, w)
def count_mat2q(m, counters):
    if counters is not None:
        if m[0] + m[4] + m[8] > 0:
            counters["mat2q_trace"] += 1
        else:
            i = 1 if m[4] > m[0] else 0
            if m[8] > m[4 * i]:
                i = 2
            counters["mat2q_diag%d" % i] += 1
    return mat2q(m)


def qnormalize(q):
    """SE3Quat::normalizeRotation."""
    x, y, z, w = q
    if w < 0:
        x, y, z, w = -x, -y, -z, -w
    n = math.sqrt(x * x + y * y + z * z + w * w)
    return (x / n, y / n, z / n, w / n)


def qmat(q):
    """QuaternionBase::toRotationMatrix, row-major list of 9."""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1 - (txx + tyy)]


def se3_exp(update, counters=None):
    """SE3Quat::exp, se3quat.h:223-257."""
    w = [float(update[0]), float(update[1]), float(update[2])]
    up = [float(update[3]), float(update[4]), float(update[5])]
    theta = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    O = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    O2 = [O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c] + O[3 * r + 2] * O[6 + c] for r in range(3) for c in range(3)]
    I = [1.0 if k % 4 == 0 else 0.0 for k in range(9)]
    if theta < 0.00001:
        if counters is not None:
            counters["exp_small_theta"] += 1
        R = [I[k] + O[k] + O2[k] for k in range(9)]
        V = list(R)
    else:
        s, c = sincos_d(theta)
        a, b, d = s / theta, (1 - c) / (theta * theta), (theta - s) / (theta * theta * theta)
        R = [I[k] + a * O[k] + b * O2[k] for k in range(9)]
        V = [I[k] + b * O[k] + d * O2[k] for k in range(9)]
    q = count_mat2q(R, counters)
    t = [V[3 * r] * up[0] + V[3 * r + 1] * up[1] + V[3 * r + 2] * up[2] for r in range(3)]
    return (qnormalize(q), t)


def se3_mul(a, b):
    """SE3Quat::operator*, se3quat.h:104-110."""
    rt = qrot(a[0], b[1])
    return (qnormalize(qmul(a[0], b[0])), [a[1][i] + rt[i] for i in range(3)])


def from_tcw(Tcw, counters=None):
    """Converter::toSE3Quat on a 4x4 float matrix."""
    T = np.asarray(Tcw, F32).reshape(4, 4)
    R = [float(T[r, c]) for r in range(3) for c in range(3)]
    return (qnormalize(count_mat2q(R, counters)), [float(T[0, 3]), float(T[1, 3]), float(T[2, 3])])


def to_tcw(T):
    """Converter::toCvMat(SE3Quat)."""
    R = qmat(T[0])
    out = np.zeros((4, 4), F32)
    for r in range(3):
        for c in range(3):
            out[r, c] = F32(R[3 * r + c])
        out[r, 3] = F32(T[1][r])
    out[3, 3] = F32(1)
    return out


# ------------------------------------------------------------------ the two OnlyPose edges
# X and obs are triples of floats or of float64 arrays (the same single operations elementwise);
# K = (fx, fy, cx, cy, bf) as Python floats.
def se3_map(T, X):
    r = qrot(T[0], X)
    return [r[i] + T[1][i] for i in range(3)]


def error_mono(T, X, obs, K):
    """EdgeSE3ProjectXYZOnlyPose::computeError."""
    p = se3_map(T, X)
    return [obs[0] - (p[0] / p[2] * K[0] + K[2]), obs[1] - (p[1] / p[2] * K[1] + K[3])]


def error_stereo(T, X, obs, K):
    """EdgeStereoSE3ProjectXYZOnlyPose::computeError: 1/z is rounded to float."""
    p = se3_map(T, X)
    invz = (1.0 / p[2]).astype(F32).astype(F64) if isinstance(p[2], np.ndarray) else float(F32(1.0 / p[2]))
    u = p[0] * invz * K[0] + K[2]
    v = p[1] * invz * K[1] + K[3]
    ur = u - K[4] * invz
    return [obs[0] - u, obs[1] - v, obs[2] - ur]


def jacobian_rows(T, X, K):
    """linearizeOplus of both edges: (J0[6], J1[6], J2[6]); the mono edge uses the first two."""
    p = se3_map(T, X)
    fx, fy, bf = K[0], K[1], K[4]
    x, y = p[0], p[1]
    iz = 1.0 / p[2]
    iz2 = iz * iz
    zero = np.zeros_like(x) if isinstance(x, np.ndarray) else 0.0
    J0 = [x * y * iz2 * fx, -(1 + (x * x * iz2)) * fx, y * iz * fx, -iz * fx, zero, x * iz2 * fx]
    J1 = [(1 + y * y * iz2) * fy, -x * y * iz2 * fy, -x * iz * fy, zero, -iz * fy, y * iz2 * fy]
    J2 = [J0[0] - bf * y * iz2, J0[1] + bf * x * iz2, J0[2], J0[3], zero, J0[5] - bf * iz2]
    return J0, J1, J2


def chain_add(values):
    """+0.0, then one addition per value, in order."""
    return functools.reduce(operator.add, values, 0.0)


def chain_sub(values):
    return functools.reduce(operator.sub, values, 0.0)


# ------------------------------------------------------------------ the optimizer
class _Graph:
    """The one-vertex graph with its unary edges, and g2o's Levenberg over it."""

    def __init__(self, prob, counters):
        self.obs = np.ascontiguousarray(prob["obs"], F32).reshape(-1, 3).astype(F64)
        self.X = np.ascontiguousarray(prob["Xw"], F32).reshape(-1, 3).astype(F64)
        self.info = np.ascontiguousarray(prob["inv_sigma2"], F32).reshape(-1).astype(F64)
        self.K = [float(F32(prob[k])) for k in ("fx", "fy", "cx", "cy", "bf")]
        self.stereo = self.obs[:, 2] >= 0  # mvuRight < 0: monocular
        dm, ds = huber_deltas()
        self.delta = np.where(self.stereo, ds, dm)
        self.dsqr = (self.delta * self.delta).astype(F32).astype(F64)  # float dsqr
        n = len(self.obs)
        self.E = np.zeros((n, 3))  # every edge's _error, as its last computeError left it
        self.act = np.arange(n)
        self.robust = True
        self.T = None
        self.counters = counters
        self.trials = 0
        self.lam, self.ni, self.nBad = 0.0, 2.0, 0
        self.last_rejected = False
        self.terms = None  # the last build()'s per-edge terms: 21 H + 6 b lists

    def compute_error(self, idx):
        """computeError of the edges idx at the vertex's estimate."""
        if len(idx) == 0:
            return
        st = self.stereo[idx]
        for kind, sel in ((0, idx[~st]), (1, idx[st])):
            if len(sel) == 0:
                continue
            X = [self.X[sel, k] for k in range(3)]
            obs = [self.obs[sel, k] for k in range(3)]
            self.counters["edge_behind_camera"] += int((se3_map(self.T, X)[2] <= 0).sum())
            e = error_stereo(self.T, X, obs, self.K) if kind else error_mono(self.T, X, obs, self.K)
            for k in range(len(e)):
                self.E[sel, k] = e[k]

    def edge_chi2(self, idx):
        E, w = self.E[idx], self.info[idx]
        two = E[:, 0] * (w * E[:, 0]) + E[:, 1] * (w * E[:, 1])
        return np.where(self.stereo[idx], two + E[:, 2] * (w * E[:, 2]), two)

    def huber(self, idx, chi):
        """RobustKernelHuber::robustify -> (rho0, rho1, outer)."""
        sq = np.sqrt(chi)
        delta, dsqr = self.delta[idx], self.dsqr[idx]
        inl = chi <= dsqr
        return np.where(inl, chi, 2 * sq * delta - dsqr), np.where(inl, 1., delta / sq), ~inl

    def chi2(self):  # activeRobustChi2
        c = self.edge_chi2(self.act)
        if self.robust:
            c = self.huber(self.act, c)[0]
        return chain_add(c.tolist())

    def build(self):  # linearizeOplus + constructQuadraticForm of every active edge, in order
        a = self.act
        J = jacobian_rows(self.T, [self.X[a, k] for k in range(3)], self.K)
        E, info, st = self.E[a], self.info[a], self.stereo[a]
        w, r1 = info, 1.0
        if self.robust:
            _, r1, outer = self.huber(a, self.edge_chi2(a))
            w = r1 * info
            self.counters["huber_outer_mono"] += int((outer & ~st).sum())
            self.counters["huber_outer_stereo"] += int((outer & st).sum())
        terms = []
        for r in range(6):
            for c in range(r, 6):
                s = (J[0][r] * w) * J[0][c]
                s = s + (J[1][r] * w) * J[1][c]
                terms.append(np.where(st, s + (J[2][r] * w) * J[2][c], s))
        for r in range(6):
            s = ((r1 * J[0][r]) * info) * E[:, 0]
            s = s + ((r1 * J[1][r]) * info) * E[:, 1]
            terms.append(np.where(st, s + ((r1 * J[2][r]) * info) * E[:, 2], s))
        self.terms = [t.tolist() for t in terms]
        up = [chain_add(t) for t in self.terms[:21]]
        self.b = [chain_sub(t) for t in self.terms[21:]]
        H = [0.0] * 36
        k = 0
        for r in range(6):
            for c in range(r, 6):
                H[6 * r + c] = H[6 * c + r] = up[k]
                k += 1
        self.H = H

    def solve(self):
        Hd = list(self.H)
        for j in range(6):
            Hd[7 * j] += self.lam
        return ldlt_solve(Hd, self.b, 6)

    def lambda_init(self):
        m = 0.0
        for j in range(6):
            m = max(abs(self.H[7 * j]), m)
        self.lam, self.ni, self.nBad = 1e-5 * m, 2.0, 0

    def iteration(self, it):  # OptimizationAlgorithmLevenberg::solve
        self.compute_error(self.act)
        currentChi = self.chi2()
        iniChi = currentChi
        self.build()
        if it == 0:
            self.lambda_init()
        rho, qmax = 0.0, 0
        while True:
            bak = self.T
            ok2, x = self.solve()
            self.trials += 1
            if ok2:
                self.T = se3_mul(se3_exp(x, self.counters), self.T)
            else:
                self.counters["solve_not_positive"] += 1
            self.compute_error(self.act)
            tempChi = self.chi2()
            scale = 0.0
            if ok2:
                for j in range(6):
                    scale += x[j] * (self.lam * x[j] + self.b[j])
            (self.lam, self.ni, currentChi, rho, qmax, self.nBad), accept, go = lm_trial(
                (self.lam, self.ni, currentChi, rho, qmax, self.nBad), tempChi, scale, ok2, cube=cube_product)
            self.last_rejected = not accept
            if not accept:
                self.T = bak  # pop; the rejected trial's errors stay in the edges
                self.counters["trial_rejected"] += 1
            if not go:
                break
        (self.lam, self.ni, currentChi, rho, qmax, self.nBad), stop = lm_iteration_end(
            (self.lam, self.ni, currentChi, rho, qmax, self.nBad), iniChi, self.counters)
        return not stop

    def optimize(self, its):
        self.last_rejected = False
        if len(self.act) == 0:
            self.counters["round_without_active_edge"] += 1
            return 0
        n = 0
        for i in range(its):
            n += 1
            if not self.iteration(i):
                return n
        self.counters["ten_iterations"] += 1
        return n


def pose_optimization(prob, counters=None):
    """Optimizer::PoseOptimization on the dict oracle.pose_optimization takes (obs[n,3] (u, v, ur; ur < 0 =
    monocular), Xw[n,3], inv_sigma2[n], fx, fy, cx, cy, bf, Tcw[4,4]).  Returns dict(Tcw[4,4] float32,
    outlier[n] uint8, ngood, iterations[4] int32, trials[4], nact[4] (active edges per round), counters)."""
    counters = collections.Counter() if counters is None else counters
    G = _Graph(prob, counters)
    n = len(G.obs)
    Tin = np.array(np.asarray(prob["Tcw"], F32).reshape(4, 4))
    outlier = np.zeros(n, np.uint8)
    out = {"Tcw": Tin, "outlier": outlier, "ngood": 0, "iterations": np.zeros(4, np.int32), "trials": [0, 0, 0, 0],
           "nact": [0, 0, 0, 0], "counters": counters}
    if n < 3:
        counters["early_lt3"] += 1
        return out
    chi2Mono, chi2Stereo = float(F32(5.991)), float(F32(7.815))
    th = np.where(G.stereo, chi2Stereo, chi2Mono)
    everyone = np.arange(n)
    nBad = 0
    with np.errstate(all="ignore"):
        T0 = from_tcw(Tin, counters)
        for it in range(4):
            G.T = T0
            G.act = everyone[outlier == 0]  # initializeOptimization(0): the level-0 edges
            out["nact"][it] = len(G.act)
            t0 = G.trials
            out["iterations"][it] = G.optimize(10)
            out["trials"][it] = G.trials - t0
            if G.last_rejected:
                counters["round_ended_on_rejected_trial"] += 1
            G.compute_error(everyone[outlier != 0])
            chi2 = G.edge_chi2(everyone).astype(F32).astype(F64)  # const float chi2 = e->chi2()
            bad = chi2 > th
            counters["outlier_reinstated"] += int(((outlier != 0) & ~bad).sum())
            outlier[:] = bad
            nBad = int(bad.sum())
            if it == 2:
                G.robust = False
            if n < 10:
                counters["one_round_lt10"] += 1
                break
    out["Tcw"] = to_tcw(G.T)
    out["ngood"] = n - nBad
    return out


def linear_step(prob, robust):
    """The first iteration's linear system at the start pose with every edge active, and its first trial:
    dict(terms (21 H + 6 b lists over the edges), chi_terms, H[36], b[6], chi, lam, ok, x[6], temp_chi (the
    chi at exp(x) * T0)) -- for the exact-arithmetic test."""
    G = _Graph(prob, collections.Counter())
    G.robust = bool(robust)
    with np.errstate(all="ignore"):
        G.T = from_tcw(prob["Tcw"])
        G.compute_error(G.act)
        c = G.edge_chi2(G.act)
        chi_terms = (G.huber(G.act, c)[0] if G.robust else c).tolist()
        chi = G.chi2()
        G.build()
        H, b = list(G.H), list(G.b)
        G.lambda_init()
        ok, x = G.solve()
        G.T = se3_mul(se3_exp(x), G.T)
        G.compute_error(G.act)
        temp_chi = G.chi2()
    return {"terms": G.terms, "chi_terms": chi_terms, "H": H, "b": b, "chi": chi, "lam": G.lam, "ok": ok, "x": x,
            "temp_chi": temp_chi}

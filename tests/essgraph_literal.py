"""A literal Python restatement of the reference's Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:888-1218)
with the g2o pieces it runs -- the yardstick of tests/test_essgraph.py.  It is not the code under test and
needs no GPU.

Every arithmetic step is one IEEE double operation, on a Python float (the vertex updates, the LM state)
or elementwise on numpy float64 arrays: over the edges (errors, the 28 perturbed errors, Jacobians,
quadratic-form terms), over a matrix row or block (assembly, the factorisation).  The sums g2o forms over
the edges run in edge insertion order.  Parity against the genuine g2o/Eigen binary is unpinned, as for
PoseOptimization and OptimizeSim3: the evaluation orders below are the ones Eigen 3's
fixed-size expression templates produce when read from their sources, written down so a later pinning has
one place to correct.  tests/optsim3_literal.py lists the orders of Sim3's constructor, operator*, inverse
and map, which are shared; the ones new here:

* Sim3::log (sim3.h:148-230): toRotationMatrix is Eigen's (orbx_lm.h qmat); d = 0.5*(((R00+R11)+R22)-1);
  deltaR and skew as se3_ops.hpp writes them; omega = (theta/(2*sqrt(1-d*d)))*deltaR resp. 0.5*deltaR;
  `A*Omega + B*Omega*Omega + C*I` is (A*Omega + ((B*Omega)*Omega)) + C*I per entry, the 3x3 product summing
  its three products left to right.
* W.lu().solve(t) is PartialPivLU at 3x3: the first largest |entry| of the column pivots (rows exchanged
  whole), the column below is DIVIDED by the pivot, the trailing block takes the outer product; then the
  permuted right-hand side goes through the unit-lower and the upper triangular solves column by column
  (x_i final, then rhs[others] -= x_i * column), the upper one dividing by the diagonal.
* std::log is log_det, acos is acos_det, sin / cos are sincos_d, std::exp is exp_det (twins of
  orbx_device.h), where the reference calls the host libm.
* EdgeSim3::computeError: (C * v0) * v1.inverse(), then log().
* linearizeOplus (base_binary_edge.hpp:131-205): per vertex that is not fixed and per d, oplus(+1e-9 e_d),
  error, pop, oplus(-1e-9 e_d), error, pop; column d = (1/(2*1e-9)) * (e_plus - e_minus).  oplusImpl zeroes
  update[6] under _fix_scale.
* constructQuadraticForm (:60-120) with information = I: the products with the identity's zeros are
  dropped and 1*x is x, so omega_r = -e, A^T*Omega = A^T.  b_v += sum_k J[k][r]*(-e_k), A_vv += sum_k
  J[k][r]*J[k][c], the off-diagonal block sum_k J0[k][r]*J1[k][c] (all left to right, formed first, then
  added to the accumulator, which starts at zero); an edge whose vertex 0 has the larger Hessian index
  adds that block to the transposed slot (_hessianTransposed) -- the same scalars.  chi2 = sum_k e_k*e_k.
* The linear solve: the reference's SimplicialLDLT runs under an AMD ordering nobody here can replay.  The
  solve here is LDL^T without pivoting in the natural order (free vertices by ascending id, 7 scalars
  each): for k ascending, d_k = a_kk (zero: the solve fails), l_ik = a_ik / d_k, a_ij -= (l_ik*d_k)*l_jk
  for k < j <= i -- written densely with numpy, one outer-product step per k; then L y = b by columns
  (y[k+1:] -= L[k+1:,k]*y_k), y / d, L^T x = y by rows from the last (y[:k] -= L[k,:k]*x_k).  Each entry
  takes its updates for k ascending (descending in the last), so the block-envelope form of the library
  produces the same bits: the entries it skips are structural zeros.
* The LM loop is tests/optsim3_literal.py's (oracle/poseopt.cpp's restatement of
  optimization_algorithm_levenberg.cpp), at 7 (n - 1) unknowns, with lambda_0 the user value 1e-16, no
  robust kernel and no stop flag.

The reference walks `std::map<KeyFrame*, ...>` and `std::set<KeyFrame*>` in pointer order, which no run
reproduces; the edge selection here walks keyframe ids in ascending order (edge order changes summation
order only).  A keyframe with the bad flag gets no vertex, an edge that would touch it is not added (g2o's
addEdge refuses a null vertex) and its pose stays; a bad point stays.

`counters` records how often each branch fired so a test can assert its input reaches them.
"""
import collections

import numpy as np

from optsim3_literal import (DBL_MAX, EPS, exp_det, lm_iteration_end, lm_trial, mat2q, qmul, qrot,  # noqa: F401
                             sim3_exp, sim3_inverse, sim3_map, sim3_mul)

F32 = np.float32
F64 = np.float64
U = 2.0 ** -53


# ------------------------------------------------------------------ twins of orbx_device.h (float or array in)
def log_det(x):
    """Twin of orbx_device.h log_det: ln x from basic IEEE operations only, for positive normal doubles.

    x = m 2^k from the exponent bits, m in (sqrt(1/2), sqrt 2] (m in [1, 2) halved when above sqrt 2: exact);
    f = m - 1 (exact: Sterbenz, m within a factor 2 of 1); s = f / (2 + f), |s| <= 0.1716;
    ln m = 2 atanh s = 2s + s*(z*P(z)), z = s*s, P = 2/3 + 2z/5 + ... + 2 z^10/23 by Horner;
    result = k*ln2_hi + (ln m + k*ln2_lo).  At x = 1: k = 0, f = 0, s = 0 and every term is 0: exactly 0.0.

    Error against the true logarithm, u = 2^-53:
      k = 0 (x = m)  2 + f rounds (u relative), the division rounds (u): s carries 2u relative; 2 atanh s
                     has relative condition (s / atanh s) / (1 - s^2) <= 1 / (1 - 0.0295) < 1.031, so 2.07u.
                     s + s is exact.  z*P is below 0.0295 * 0.68 = 0.0201 of s and carries z's 5u, P's
                     Horner error (< 3u) and two roundings: under 10u of a term that is at most 1.01 % of the
                     result, 0.11u.  Truncation: 2 s^25 / 25 against 2s is s^24 / 25 < 1.7e-20 = 0.0002u.
                     The final sum rounds once: u.  Total < 3.2u, counted as 4u |ln m|.
      k != 0         |ln x| >= ln sqrt 2 = 0.3466.  k*ln2_hi is exact (ln2_hi has 21 trailing zero bits,
                     |k| < 2^11); ln2_hi + ln2_lo misses ln 2 by < 2^-102 (times |k| <= 1074: negligible);
                     k*ln2_lo rounds below 2^-75; ln m + k*ln2_lo rounds half an ulp below 0.5: 2^-55 =
                     0.25u absolute; ln m's own error is 4u * 0.3466 = 1.39u absolute; the outer sum rounds
                     u relative.  (1.39 + 0.25)u / 0.3466 + u = 5.74u.
    |log_det(x) - ln x| <= 6u |ln x| = LOG_DET_BOUND, every positive normal x.
    """
    x = np.asarray(x, F64)
    with np.errstate(all="ignore"):
        ok = (x >= 2.2250738585072014e-308) & (x <= 1.7976931348623157e308)
        xs = np.where(ok, x, 1.0)
        bits = np.atleast_1d(xs).view(np.int64).reshape(xs.shape)
        k = ((bits >> 52) & 0x7ff) - 1023
        m = np.atleast_1d((bits & 0x000fffffffffffff) | 0x3ff0000000000000).view(F64).reshape(xs.shape)
        big = m > 1.41421356237309514547e+00
        m = np.where(big, m * 0.5, m)
        kd = (k + big).astype(F64)
        f = m - 1.0
        s = f / (2.0 + f)
        z = s * s
        p = 2.0 / 23.0
        for c in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
            p = p * z + 2.0 / c
        lm = (s + s) + s * (z * p)
        r = kd * 6.93147180369123816490e-01 + (lm + kd * 1.90821492927058770002e-10)
        r = np.where(ok, r, np.nan)
    return r if r.ndim else float(r)


LOG_DET_BOUND = 6 * U  # relative (derived in log_det's docstring)


def atan2_det(y, x):
    """Array twin of orbx_device.h atan2_det (tests/sim3_literal.py holds the scalar one; a test pins the two
    to each other)."""
    y, x = np.asarray(y, F64), np.asarray(x, F64)
    with np.errstate(all="ignore"):
        nan = (y != y) | (x != x)
        ny, nx = np.signbit(y), np.signbit(x)
        ay, ax = np.where(ny, -y, y), np.where(nx, -x, x)
        sw = ay > ax
        hi, lo = np.where(sw, ay, ax), np.where(sw, ax, ay)
        t = np.where(hi == 0.0, 0.0, np.where(lo == hi, 1.0, lo / np.where(hi == 0.0, 1.0, hi)))
        k = np.rint(t * 4.0)
        c = k * 0.25
        base = np.where(k == 0.0, 0.0, np.where(k == 1.0, 2.44978663126864143e-01, np.where(
            k == 2.0, 4.63647609000806094e-01, np.where(k == 3.0, 6.43501108793284371e-01, 7.85398163397448279e-01))))
        r = (t - c) / (1.0 + t * c)
        r2 = r * r
        p = 1.0 / 23.0
        for sg, cc in ((-1, 21.0), (1, 19.0), (-1, 17.0), (1, 15.0), (-1, 13.0), (1, 11.0), (-1, 9.0), (1, 7.0),
                       (-1, 5.0), (1, 3.0)):
            p = p * r2 - 1.0 / cc if sg < 0 else p * r2 + 1.0 / cc
        a = base + (r - r * (r2 * p))
        a = np.where(sw, (1.57079632679489656e+00 - a) + 6.12323399573676604e-17, a)
        a = np.where(nx, (3.14159265358979312e+00 - a) + 1.22464679914735321e-16, a)
        a = np.where(ny, -a, a)
        a = np.where(nan, y + x, a)
    return a if a.ndim else float(a)


def acos_det(x):
    """Twin of orbx_device.h acos_det: acos x = atan2_det(sqrt((1 - x)*(1 + x)), x); |x| > 1 gives NaN, -0
    counts as +0, acos_det(1) is exactly 0.

    Error against the true arc cosine on [-1, 1), u = 2^-53.  y = sqrt((1-x)(1+x)): 1 - x and 1 + x round
    (u each; 1 - x is exact for x >= 0.5), the product rounds (u), the root halves the 3u and rounds (u):
    y carries 2.5u relative.  atan2(y, x) = theta has d theta = sin(theta) cos(theta) dy/y, and
    sin cos / theta <= 1: 2.5u relative.  atan2_det itself, first octant angle phi = atan t, t = lo/hi:
    t rounds (u): u t / (1 + t^2) <= 0.5u absolute; t - c is exact (c = 0, or Sterbenz: t in [c/2, 2c]);
    1 + t*c rounds twice, the division once: r carries 3u relative, |r| <= 1/8; r - r*(r2*p) adds under
    1.2u relative: 4.2u |r| <= 0.53u absolute; base is within half an ulp of atan c (0.39u absolute at most)
    and base + (...) rounds u relative.  For k = 0 the angle is r's series and all of it is relative: 5.2u.
    For k >= 1 the angle is at least atan(1/8) = 0.1244: (0.5 + 0.53 + 0.39)u / 0.1244 + u = 12.4u.  So 13u
    on phi <= pi/4.  The fold (pi/2_hi - a) + pi/2_lo, result in [pi/4, pi/2]: 13u * 0.7854 = 10.2u absolute
    plus two roundings (0.79u each): 11.8u / 0.7854 = 15u.  The fold (pi_hi - a) + pi_lo, result >= pi/2:
    15u * 1.571 = 23.6u absolute plus two roundings (1.57u each): 26.7u / 1.571 = 17u.  With y's 2.5u:
    |acos_det(x) - acos x| <= 20u acos x = ACOS_DET_BOUND.
    """
    x = np.asarray(x, F64)
    with np.errstate(all="ignore"):
        x = np.where(x == 0.0, 0.0, x)
        r = atan2_det(np.sqrt((1.0 - x) * (1.0 + x)), x)
    return r


ACOS_DET_BOUND = 20 * U  # relative on [-1, 1) (derived in acos_det's docstring)


def sincos_d(x):
    """Array twin of orbx_device.h sincos_d (tests/sim3_literal.py holds the scalar one)."""
    x = np.asarray(x, F64)
    with np.errstate(all="ignore"):
        kd = np.rint(x * 6.36619772367581382433e-01)
        q = np.where(np.isfinite(kd), kd, 0.0).astype(np.int64) & 3
        r = (x - kd * 1.57079632673412561417e+00) - kd * 6.07710050650619224932e-11
        r2 = r * r
        ps = 1.0 / 51090942171709440000.0
        for sg, c in ((-1, 121645100408832000.0), (1, 355687428096000.0), (-1, 1307674368000.0), (1, 6227020800.0),
                      (-1, 39916800.0), (1, 362880.0), (-1, 5040.0), (1, 120.0), (-1, 6.0)):
            ps = ps * r2 - 1.0 / c if sg < 0 else ps * r2 + 1.0 / c
        sr = r + r * (r2 * ps)
        pc = 1.0 / 2432902008176640000.0
        for sg, c in ((-1, 6402373705728000.0), (1, 20922789888000.0), (-1, 87178291200.0), (1, 479001600.0),
                      (-1, 3628800.0), (1, 40320.0), (-1, 720.0), (1, 24.0)):
            pc = pc * r2 - 1.0 / c if sg < 0 else pc * r2 + 1.0 / c
        pc = pc * r2 - 0.5
        cr = 1.0 + r2 * pc
        s = np.where(q == 0, sr, np.where(q == 1, cr, np.where(q == 2, -sr, -cr)))
        c = np.where(q == 0, cr, np.where(q == 1, -sr, np.where(q == 2, -cr, sr)))
    return s, c


def qmat(q):
    """Quaterniond::toRotationMatrix (orbx_lm.h qmat) -> row-major list of 9."""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1 - (txx + tyy)]


LOG_BRANCHES = ("log_small_sigma_small_rot", "log_small_sigma_rot", "log_sigma_small_rot", "log_sigma_rot")


def _cswap(sw, a, b):
    return np.where(sw, b, a), np.where(sw, a, b)


def sim3_log(S, counters=None, want_branch=False):
    """Sim3::log(), sim3.h:148-230, on a Sim3 of floats or of arrays -> list of 7 (omega, upsilon, sigma).
    With want_branch also the probe's branch word (bit 0: d <= 1 - eps, bit 1: |sigma| >= eps, bit 2 / 3: a
    row exchange at the first / second pivot)."""
    q, t, s = S
    q = tuple(np.asarray(v, F64) for v in q)
    t = [np.asarray(v, F64) for v in t]
    s = np.asarray(s, F64)
    with np.errstate(all="ignore"):
        sigma = np.asarray(log_det(s), F64)
        R = qmat(q)
        d = 0.5 * (R[0] + R[4] + R[8] - 1)
        dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
        small_sigma = np.abs(sigma) < EPS
        small_rot = d > 1 - EPS
        theta = np.asarray(acos_det(d), F64)
        f = theta / (2 * np.sqrt(1 - d * d))
        om = [np.where(small_rot, 0.5 * v, f * v) for v in dR]
        sn, cs = sincos_d(theta)
        theta2 = theta * theta
        sigma2 = sigma * sigma
        # |sigma| < eps
        A1 = np.where(small_rot, 1. / 2., (1 - cs) / theta2)
        B1 = np.where(small_rot, 1. / 6., (theta - sn) / (theta2 * theta))
        # else
        C2 = (s - 1) / sigma
        a, b = s * sn, s * cs
        c = theta2 + sigma * sigma
        A2 = np.where(small_rot, ((sigma - 1) * s + 1) / sigma2, (a * sigma + (1 - b) * theta) / (theta * c))
        B2 = np.where(small_rot, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma),
                      (C2 - ((b - 1) * sigma + a * theta) / c) * 1. / theta2)
        A = np.where(small_sigma, A1, A2)
        B = np.where(small_sigma, B1, B2)
        C = np.where(small_sigma, 1.0, C2)
        z = np.zeros_like(om[0])
        O = [z, -om[2], om[1], om[2], z, -om[0], -om[1], om[0], z]
        BO = [B * v for v in O]
        W = []
        for r in range(3):
            for cc in range(3):
                p = BO[3 * r] * O[cc] + BO[3 * r + 1] * O[3 + cc] + BO[3 * r + 2] * O[6 + cc]
                W.append(A * O[3 * r + cc] + p + C * (1.0 if r == cc else 0.0))
        y = list(t)
        # pivot 0
        big = np.zeros(np.shape(W[0]), np.int64)
        bv = np.abs(W[0])
        g = np.abs(W[3]) > bv
        bv, big = np.where(g, np.abs(W[3]), bv), np.where(g, 1, big)
        g = np.abs(W[6]) > bv
        bv, big = np.where(g, np.abs(W[6]), bv), np.where(g, 2, big)
        for cc in range(3):
            W[cc], W[3 + cc] = _cswap(big == 1, W[cc], W[3 + cc])
            W[cc], W[6 + cc] = _cswap(big == 2, W[cc], W[6 + cc])
        y[0], y[1] = _cswap(big == 1, y[0], y[1])
        y[0], y[2] = _cswap(big == 2, y[0], y[2])
        nz = bv != 0.0
        W[3] = np.where(nz, W[3] / W[0], W[3])
        W[6] = np.where(nz, W[6] / W[0], W[6])
        W[4] = W[4] - W[3] * W[1]
        W[5] = W[5] - W[3] * W[2]
        W[7] = W[7] - W[6] * W[1]
        W[8] = W[8] - W[6] * W[2]
        # pivot 1
        sw = np.abs(W[7]) > np.abs(W[4])
        for cc in range(3):
            W[3 + cc], W[6 + cc] = _cswap(sw, W[3 + cc], W[6 + cc])
        y[1], y[2] = _cswap(sw, y[1], y[2])
        W[7] = np.where(W[4] != 0.0, W[7] / W[4], W[7])
        W[8] = W[8] - W[7] * W[5]
        y[1] = y[1] - y[0] * W[3]
        y[2] = y[2] - y[0] * W[6]
        y[2] = y[2] - y[1] * W[7]
        y[2] = y[2] / W[8]
        y[0] = y[0] - y[2] * W[2]
        y[1] = y[1] - y[2] * W[5]
        y[1] = y[1] / W[4]
        y[0] = y[0] - y[1] * W[1]
        y[0] = y[0] / W[0]
    br = (np.where(small_rot, 0, 1) | np.where(small_sigma, 0, 2) | np.where(big != 0, 4, 0) | np.where(sw, 8, 0))
    if counters is not None:
        bw = np.atleast_1d(br)
        for k in range(4):
            counters[LOG_BRANCHES[k]] += int(((bw & 3) == k).sum())
        counters["lu_swap_first"] += int(((bw & 4) != 0).sum())
        counters["lu_swap_second"] += int(((bw & 8) != 0).sum())
        counters["lu_no_swap"] += int(((bw & 12) == 0).sum())
    res = [om[0], om[1], om[2], y[0], y[1], y[2], sigma + z]
    return (res, br) if want_branch else res


def sim3_cols(A):
    """n x 8 array -> Sim3 of column arrays."""
    A = np.asarray(A, F64).reshape(-1, 8)
    return ((A[:, 0], A[:, 1], A[:, 2], A[:, 3]), [A[:, 4], A[:, 5], A[:, 6]], A[:, 7])


def sim3_rows(S, n):
    return np.stack([np.broadcast_to(np.asarray(v, F64), (n,)) for v in list(S[0]) + list(S[1]) + [S[2]]], axis=1).copy()


def sim3_take(S, idx):
    return (tuple(v[idx] for v in S[0]), [v[idx] for v in S[1]], S[2][idx])


def sim3_from_tcw(Tcw):
    """Converter::toMatrix3d / toVector3d + g2o::Sim3(R, t, 1.0) (orbx_sim3_from_tcw) -> 8 doubles."""
    T = np.asarray(Tcw, F32).reshape(-1)[:12].reshape(3, 4).astype(F64)
    return np.array(list(mat2q([float(v) for v in T[:, :3].reshape(9)])) + [float(v) for v in T[:, 3]] + [1.0], F64)


DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)


def edge_error(C, v0, v1, counters=None):
    return sim3_log(sim3_mul(sim3_mul(C, v0), sim3_inverse(v1)), counters)


def measurements(P):
    """Sji = Sjw * Swi from the table the edge's kind selects -> E x 8."""
    E = len(P["edge_v0"])
    kind = np.asarray(P["edge_kind"]).astype(bool)
    tab = np.where(kind[:, None, None], np.asarray(P["Snc"], F64)[None], np.asarray(P["Scw"], F64)[None]) \
        if E else np.zeros((0, len(P["Scw"]), 8))
    ar = np.arange(E)
    Si = sim3_cols(tab[ar, P["edge_v0"]]) if E else sim3_cols(np.zeros((0, 8)))
    Sj = sim3_cols(tab[ar, P["edge_v1"]]) if E else sim3_cols(np.zeros((0, 8)))
    return sim3_rows(sim3_mul(Sj, sim3_inverse(Si)), E)


# ------------------------------------------------------------------ the linear solve
def ldlt_solve(H, b, lam):
    """(H + lam I) x = b by the recurrence of the module docstring; H dense symmetric (its lower triangle
    is read).  Returns (ok, x); ok is False on an exactly zero pivot."""
    a = np.array(H, F64)
    n = len(a)
    a[np.arange(n), np.arange(n)] += lam
    d = np.zeros(n)
    with np.errstate(all="ignore"):
        for k in range(n):
            dk = a[k, k]
            if dk == 0.0:
                return False, np.zeros(n)
            d[k] = dk
            l = a[k + 1:, k] / dk
            w = l * dk
            a[k + 1:, k + 1:] -= np.outer(w, l)  # (only the lower triangle is read later)
            a[k + 1:, k] = l
        y = np.array(b, F64)
        for k in range(n):
            y[k + 1:] -= a[k + 1:, k] * y[k]
        y = y / d
        for k in range(n - 1, -1, -1):
            y[:k] -= a[k, :k] * y[k]
    return True, y


# ------------------------------------------------------------------ the graph
class Graph:
    def __init__(self, P, counters):
        self.P = P
        self.c = counters
        self.n = len(P["Scw"])
        self.fixed = int(P["fixed_vertex"])
        self.fix = bool(P["bFixScale"])
        self.ev0 = np.asarray(P["edge_v0"], np.int64)
        self.ev1 = np.asarray(P["edge_v1"], np.int64)
        self.E = len(self.ev0)
        self.meas = measurements(P)
        self.C = sim3_cols(self.meas)
        self.est = np.array(P["Scw"], F64).reshape(-1, 8).copy()
        self.hidx = np.full(self.n, -1, np.int64)
        free = [v for v in range(self.n) if v != self.fixed]
        self.hidx[free] = np.arange(len(free))
        self.hv = np.array(free, np.int64)
        self.N = 7 * len(free)
        self.trials = 0
        self.fails = 0
        self.lam, self.ni, self.nBad = 0.0, 2.0, 0
        seen = set()
        for a, b in zip(self.hidx[self.ev0], self.hidx[self.ev1]):
            if a < 0 or b < 0:
                continue
            if a > b:
                counters["transposed_block"] += 1
            key = (max(a, b), min(a, b))
            if key in seen:
                counters["duplicate_pair_block"] += 1
            seen.add(key)

    def errors(self, count=False):  # computeActiveErrors -> E x 7
        e = edge_error(self.C, sim3_cols(self.est[self.ev0]), sim3_cols(self.est[self.ev1]), self.c if count else None)
        return np.stack([np.broadcast_to(v, (self.E,)) for v in e], axis=1) if self.E else np.zeros((0, 7))

    def chi2(self, err):
        s = 0.0
        if self.E:
            t = err[:, 0] * err[:, 0]
            for k in range(1, 7):
                t = t + err[:, k] * err[:, k]
            for v in t.tolist():
                s = s + v
        return s

    def jacobians(self):
        """linearizeOplus of every edge: J0, J1 as E x 7 x 7 ([edge][error entry][d]); zero for a fixed vertex."""
        J = [np.zeros((self.E, 7, 7)), np.zeros((self.E, 7, 7))]
        v = [sim3_cols(self.est[self.ev0]), sim3_cols(self.est[self.ev1])]
        for side in range(2):
            fx = (self.ev0 if side == 0 else self.ev1) == self.fixed
            for d in range(7):
                pm = []
                for step in (DELTA, -DELTA):
                    add = [0.0] * 7
                    add[d] = step
                    if self.fix:
                        add[6] = 0.0
                    pert = sim3_mul(sim3_exp(add), v[side])
                    e = edge_error(self.C, pert if side == 0 else v[0], pert if side == 1 else v[1])
                    pm.append(np.stack([np.broadcast_to(x, (self.E,)) for x in e], axis=1))
                col = SCALAR * (pm[0] - pm[1])
                J[side][:, :, d] = np.where(fx[:, None], 0.0, col)
        return J

    def build(self, err):
        """buildSystem at the current estimates: H (dense, both triangles), b."""
        J0, J1 = self.jacobians()
        E, N = self.E, self.N

        def prod(A, B):  # sum_k A[k][r]*B[k][c], left to right
            t = A[:, 0, :, None] * B[:, 0, None, :]
            for k in range(1, 7):
                t = t + A[:, k, :, None] * B[:, k, None, :]
            return t

        def vec(A):
            t = A[:, 0, :] * (-err[:, 0, None])
            for k in range(1, 7):
                t = t + A[:, k, :] * (-err[:, k, None])
            return t
        if E:
            A00, A01, A11, b0, b1 = prod(J0, J0), prod(J0, J1), prod(J1, J1), vec(J0), vec(J1)
        H = np.zeros((N, N))
        b = np.zeros(N)
        for e in range(E):
            h0, h1 = int(self.hidx[self.ev0[e]]), int(self.hidx[self.ev1[e]])
            if h0 >= 0:
                H[7 * h0:7 * h0 + 7, 7 * h0:7 * h0 + 7] += A00[e]
                b[7 * h0:7 * h0 + 7] += b0[e]
            if h1 >= 0:
                H[7 * h1:7 * h1 + 7, 7 * h1:7 * h1 + 7] += A11[e]
                b[7 * h1:7 * h1 + 7] += b1[e]
            if h0 >= 0 and h1 >= 0:
                H[7 * h0:7 * h0 + 7, 7 * h1:7 * h1 + 7] += A01[e]
                H[7 * h1:7 * h1 + 7, 7 * h0:7 * h0 + 7] += A01[e].T
        self.J0, self.J1 = J0, J1
        self.H, self.b = H, b

    def update(self, x):
        """SparseOptimizer::update: oplus of every free vertex; x[6] of each is zeroed in place under
        _fix_scale."""
        for h, v in enumerate(self.hv):
            u = [float(a) for a in x[7 * h:7 * h + 7]]
            if self.fix:
                u[6] = 0.0
                x[7 * h + 6] = 0.0
                self.c["fix_scale_zeroing"] += 1
            S = (tuple(float(a) for a in self.est[v, :4]), [float(a) for a in self.est[v, 4:7]], float(self.est[v, 7]))
            r = sim3_mul(sim3_exp(u, self.c), S)
            self.est[v] = list(r[0]) + list(r[1]) + [r[2]]

    def iteration(self, it, lambda_init):
        err = self.errors(count=True)
        currentChi = self.chi2(err)
        iniChi = currentChi
        if it == 0:
            self.chi0 = currentChi
            self.err0 = err
        self.build(err)
        if it == 0:
            self.lam = float(lambda_init)  # setUserLambdaInit: computeLambdaInit returns the user's value
            self.ni, self.nBad = 2.0, 0
            self.H0, self.b0 = self.H.copy(), self.b.copy()
        rho, qmax = 0.0, 0
        while True:
            bak = self.est.copy()
            ok2, x = ldlt_solve(self.H, self.b, self.lam)
            self.trials += 1
            if ok2:
                self.update(x)
            else:
                self.fails += 1
                self.c["solver_failures"] += 1
            tempChi = self.chi2(self.errors())
            scale = 0.0
            if ok2:
                for v in (x * (self.lam * x + self.b)).tolist():
                    scale = scale + v
            (self.lam, self.ni, currentChi, rho, qmax, self.nBad), accept, go = lm_trial(
                (self.lam, self.ni, currentChi, rho, qmax, self.nBad), tempChi, scale, ok2)
            if not accept:
                self.est = bak
                self.c["rejected_trials"] += 1
            if not go:
                break
        self.chi = currentChi
        (self.lam, self.ni, currentChi, rho, qmax, self.nBad), stop = lm_iteration_end(
            (self.lam, self.ni, currentChi, rho, qmax, self.nBad), iniChi)
        return not stop

    def optimize(self, its, lambda_init):
        n = 0
        self.chi0 = self.chi = 0.0
        for i in range(its):
            n += 1
            if not self.iteration(i, lambda_init):
                self.c["stop_rule"] += 1
                return n
        if its:
            self.c["iteration_cap"] += 1
        return n


def run_problem(P, counters=None):
    """The optimisation and the write-back on a gathered problem: dict(vertex_id[n], Scw[n,8], Snc[n,8],
    fixed_vertex, bFixScale, edge_v0, edge_v1, edge_kind, iterations, lambda_init, Xw[m,3] float32,
    point_ref[m]).  Returns dict(Scw_out[n,8], Tcw_out[n,12] float32, Xw_out[m,3] float32, iterations,
    trials, chi2_initial, chi2_final, solver_failures, counters, graph)."""
    counters = collections.Counter() if counters is None else counters
    G = Graph(P, counters)
    with np.errstate(all="ignore"):
        its = G.optimize(int(P["iterations"]), float(P["lambda_init"]))
        S = sim3_cols(G.est)
        R = qmat(S[0])
        inv_s = 1. / S[2]
        T = np.zeros((G.n, 12), F32)
        for r in range(3):
            for c in range(3):
                T[:, 4 * r + c] = R[3 * r + c].astype(F32)
            T[:, 4 * r + 3] = (S[1][r] * inv_s).astype(F32)
        X = np.ascontiguousarray(P["Xw"], F32).reshape(-1, 3)
        ref = np.asarray(P["point_ref"], np.int64).reshape(-1)
        if len(X):
            Srw = sim3_take(sim3_cols(P["Scw"]), ref)
            Swr = sim3_take(sim3_inverse(S), ref)
            Xd = X.astype(F64)
            c = sim3_map(Swr, sim3_map(Srw, [Xd[:, 0], Xd[:, 1], Xd[:, 2]]))
            Xo = np.stack(c, axis=1).astype(F32)
        else:
            Xo = np.zeros((0, 3), F32)
    return {"Scw_out": G.est.copy(), "Tcw_out": T, "Xw_out": Xo, "iterations": its, "trials": G.trials,
            "chi2_initial": G.chi0, "chi2_final": G.chi, "solver_failures": G.fails, "counters": counters, "graph": G}


# ------------------------------------------------------------------ the caller's side (:913-1138, :1144-1217)
def select_edges(M, counters=None):
    """The reference's edge selection on the map description of Optimizer.OptimizeEssentialGraph, walking
    ids in ascending order.  Returns [(nIDi, nIDj, kind)] in insertion order."""
    counters = collections.Counter() if counters is None else counters
    minFeat = 100
    KF = {kf["id"]: kf for kf in M["keyframes"]}
    good = {i for i, kf in KF.items() if not kf["bad"]}
    cur, loop = M["pCurKF"], M["pLoopKF"]
    weight = {i: dict(kf["covisibles"]) for i, kf in KF.items()}
    edges, inserted = [], set()
    for i in sorted(M["LoopConnections"]):
        for j in sorted(M["LoopConnections"][i]):
            if (i != cur or j != loop) and weight[i].get(j, 0) < minFeat:
                continue
            if (i == cur and j == loop) and weight[i].get(j, 0) < minFeat:
                counters["minfeat_exception"] += 1
            if i in good and j in good:
                edges.append((i, j, 0))
            inserted.add((min(i, j), max(i, j)))
    for i in sorted(KF):
        kf = KF[i]
        if i not in good:
            continue
        parent = kf["parent"]
        if parent is not None and parent in good:
            edges.append((i, parent, 1))
        loops = set(kf["loop_edges"])
        for l in sorted(loops):
            if l < i and l in good:
                edges.append((i, l, 1))
        # GetCovisiblesByWeight(minFeat): the ordered list up to the first weight below minFeat; the
        # reference returns an empty list when there is none (its upper_bound reaches end())
        below = [k for k, (_, w) in enumerate(kf["covisibles"]) if w < minFeat]
        for j, w in kf["covisibles"][:below[0] if below else 0]:
            if j != parent and j not in kf["children"] and j not in loops:
                if not KF[j]["bad"] and j < i:
                    if (min(i, j), max(i, j)) in inserted:
                        counters["inserted_edges_skip"] += 1
                        continue
                    edges.append((i, j, 1))
    return edges


def gather(M, counters=None):
    """The map description -> (problem, vertex ids, indices of the points it moves)."""
    kfs = sorted((kf for kf in M["keyframes"] if not kf["bad"]), key=lambda k: k["id"])
    ids = [kf["id"] for kf in kfs]
    index = {i: k for k, i in enumerate(ids)}
    Scw = np.array([np.asarray(M["CorrectedSim3"][kf["id"]], F64) if kf["id"] in M["CorrectedSim3"]
                    else sim3_from_tcw(kf["Tcw"]) for kf in kfs], F64).reshape(-1, 8)
    Snc = np.array([np.asarray(M["NonCorrectedSim3"][kf["id"]], F64) if kf["id"] in M["NonCorrectedSim3"] else Scw[k]
                    for k, kf in enumerate(kfs)], F64).reshape(-1, 8)
    edges = select_edges(M, counters)
    pts, Xw, ref = [], [], []
    for k, mp in enumerate(M["points"]):
        if mp["bad"]:
            continue
        r = mp["mnCorrectedReference"] if mp["mnCorrectedByKF"] == M["pCurKF"] else mp["ref"]
        if r not in index:
            continue
        pts.append(k)
        Xw.append(np.asarray(mp["pos"], F32))
        ref.append(index[r])
    P = {"vertex_id": np.array(ids, np.int32), "Scw": Scw, "Snc": Snc, "fixed_vertex": index[M["pLoopKF"]],
         "bFixScale": bool(M["bFixScale"]), "edge_v0": np.array([index[e[0]] for e in edges], np.int32),
         "edge_v1": np.array([index[e[1]] for e in edges], np.int32),
         "edge_kind": np.array([e[2] for e in edges], np.uint8), "iterations": 20, "lambda_init": 1e-16,
         "Xw": np.array(Xw, F32).reshape(-1, 3), "point_ref": np.array(ref, np.int32)}
    return P, ids, pts


def optimize_essential_graph(M, counters=None):
    """Optimizer::OptimizeEssentialGraph on the map description.  Returns dict(Tcw {id: 3x4 float32} of the
    keyframes SetPose reaches, pos {point index: 3 float32} of the points SetWorldPos reaches, and
    run_problem's outputs)."""
    counters = collections.Counter() if counters is None else counters
    P, ids, pts = gather(M, counters)
    r = run_problem(P, counters)
    r["problem"] = P
    r["Tcw"] = {i: r["Tcw_out"][k].reshape(3, 4) for k, i in enumerate(ids)}
    r["pos"] = {k: r["Xw_out"][j] for j, k in enumerate(pts)}
    return r

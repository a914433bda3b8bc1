// orbx_lm.h -- the device pieces the single-vertex g2o Levenberg kernels share (poseopt.hip's SE3
// vertex, optsim3.hip's Sim3 vertex): Eigen's quaternion product / rotation / matrix conversions and
// the Eigen::LDLT<MatrixXd> restatement of oracle/poseopt.cpp, as a template on the system size;
// and the Levenberg step itself (lm::Step, start / trial / iteration_end), which essgraph.hip's pose
// graph and LocalBA's device control (ba_lm.h) run too, with the upper-triangle scatter of the
// single-vertex kernels.
// The operation sequences are the oracle's; nothing here may be re-associated.
#pragma once
#include <hip/hip_runtime.h>

namespace orbx {
namespace lm {

struct Quat {
  double x, y, z, w;
};

__device__ __forceinline__ Quat qmul(const Quat& a, const Quat& b) {
  Quat r;
  r.w = a.w * b.w - (a.x * b.x + a.y * b.y + a.z * b.z);
  r.x = a.w * b.x + b.w * a.x + (a.y * b.z - a.z * b.y);
  r.y = a.w * b.y + b.w * a.y + (a.z * b.x - a.x * b.z);
  r.z = a.w * b.z + b.w * a.z + (a.x * b.y - a.y * b.x);
  return r;
}
__device__ __forceinline__ void qrot(const Quat& q, const double v[3], double out[3]) {
  double uv[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
  uv[0] += uv[0];
  uv[1] += uv[1];
  uv[2] += uv[2];
  const double c[3] = {q.y * uv[2] - q.z * uv[1], q.z * uv[0] - q.x * uv[2], q.x * uv[1] - q.y * uv[0]};
#pragma unroll
  for (int i = 0; i < 3; i++) out[i] = v[i] + q.w * uv[i] + c[i];
}
__device__ __forceinline__ void qmat(const Quat& q, double R[9]) {
  const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}
// (also on the host: orbx_sim3_from_tcw forms g2o::Sim3(R, t, 1.0)'s quaternion there)
__host__ __device__ __forceinline__ Quat mat2q(const double m[9]) {
  Quat q;
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = __builtin_sqrt(t + 1.0);
    q.w = 0.5 * t;
    t = 0.5 / t;
    q.x = (m[7] - m[5]) * t;
    q.y = (m[2] - m[6]) * t;
    q.z = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > (i == 0 ? m[0] : m[4])) i = 2;
    // the three cases spelled out on named entries: no array indexed at run time (which put the
    // matrix in scratch memory); same arithmetic as c[i], c[j], c[k] with (i, j, k) cyclic
    if (i == 0) {  // (0, 1, 2)
      t = __builtin_sqrt(m[0] - m[4] - m[8] + 1.0);
      const double ci = 0.5 * t;
      t = 0.5 / t;
      q.w = (m[7] - m[5]) * t;
      q.x = ci;
      q.y = (m[3] + m[1]) * t;
      q.z = (m[6] + m[2]) * t;
    } else if (i == 1) {  // (1, 2, 0)
      t = __builtin_sqrt(m[4] - m[8] - m[0] + 1.0);
      const double ci = 0.5 * t;
      t = 0.5 / t;
      q.w = (m[2] - m[6]) * t;
      q.y = ci;
      q.z = (m[7] + m[5]) * t;
      q.x = (m[1] + m[3]) * t;
    } else {  // (2, 0, 1)
      t = __builtin_sqrt(m[8] - m[0] - m[4] + 1.0);
      const double ci = 0.5 * t;
      t = 0.5 / t;
      q.w = (m[3] - m[1]) * t;
      q.z = ci;
      q.x = (m[2] + m[6]) * t;
      q.y = (m[5] + m[7]) * t;
    }
  }
  return q;
}
__device__ __forceinline__ void qnormalize(Quat& q) {
  if (q.w < 0) {
    q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w;
  }
  const double n = __builtin_sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  q.x /= n; q.y /= n; q.z /= n; q.w /= n;
}

// Eigen::LDLT<MatrixXd> (diagonal pivoting) + solve at N unknowns; false when !isPositive().
// Every loop is unrolled and the pivot swaps / the permutation of the right-hand side run as
// unrolled compare-and-swap over the candidate rows, so every index is a compile-time constant:
// the matrix lives in registers (a runtime index put it in scratch memory, ~25k cycles per call
// on the LM's serial path).  Same operations in the same order as oracle/poseopt.cpp's ldlt6.
// conditional exchange of two registers by value selects (a branch per candidate let the
// compiler merge the paths into pointer phis, which sends the array to scratch memory)
__device__ __forceinline__ void cswap(bool sw, double& a, double& b) {
  const double x = a, y = b;
  a = sw ? y : x;
  b = sw ? x : y;
}
template <int N, int K, int C>
__device__ __forceinline__ void ldlt_swap(double (&m)[N * N], bool sw) {  // transpositions k <-> c (c > k)
#pragma unroll
  for (int j = 0; j < K; j++) cswap(sw, m[N * K + j], m[N * C + j]);
#pragma unroll
  for (int i = C + 1; i < N; i++) cswap(sw, m[N * i + K], m[N * i + C]);
  cswap(sw, m[(N + 1) * K], m[(N + 1) * C]);
#pragma unroll
  for (int i = K + 1; i < C; i++) cswap(sw, m[N * i + K], m[N * C + i]);
}
template <int N, int K, int C>
__device__ __forceinline__ void ldlt_swap_to(double (&m)[N * N], int big) {
  if constexpr (C < N) {
    ldlt_swap<N, K, C>(m, big == C);
    ldlt_swap_to<N, K, C + 1>(m, big);
  }
}
template <int N, int K>
__device__ __forceinline__ void ldlt_step(double (&m)[N * N], int (&tr)[N], int& sign, bool& zero) {
  if constexpr (K < N) {
    if (!zero) {
      int big = K;
      double bv = __builtin_fabs(m[(N + 1) * K]);
#pragma unroll
      for (int i = K + 1; i < N; i++)
        if (__builtin_fabs(m[(N + 1) * i]) > bv) {
          bv = __builtin_fabs(m[(N + 1) * i]);
          big = i;
        }
      if (K == 0 && !(bv > 0.0)) {
#pragma unroll
        for (int j = 0; j < N; j++) tr[j] = j;
#pragma unroll
        for (int j = 0; j < N; j++) m[(N + 1) * j] = 0.0;
        sign = 0;
        zero = true;
      } else {
        tr[K] = big;
        ldlt_swap_to<N, K, K + 1>(m, big);
        if constexpr (K > 0) {
          double temp[N];
#pragma unroll
          for (int j = 0; j < K; j++) temp[j] = m[(N + 1) * j] * m[N * K + j];
          double dot = m[N * K] * temp[0];
#pragma unroll
          for (int j = 1; j < K; j++) dot = dot + m[N * K + j] * temp[j];
          m[(N + 1) * K] -= dot;
#pragma unroll
          for (int i = K + 1; i < N; i++) {
            double sv = m[N * i] * temp[0];
#pragma unroll
            for (int j = 1; j < K; j++) sv = sv + m[N * i + j] * temp[j];
            m[N * i + K] -= sv;
          }
        }
        const double akk = m[(N + 1) * K];
        if (__builtin_fabs(akk) > 0.0) {
#pragma unroll
          for (int i = K + 1; i < N; i++) m[N * i + K] /= akk;
        }
        if (akk > 0) sign = (sign == 2 || sign == 3) ? 3 : 1;
        else if (akk < 0) sign = (sign == 1 || sign == 3) ? 3 : 2;
      }
    }
    ldlt_step<N, K + 1>(m, tr, sign, zero);
  }
}
// y[k] <-> y[t] for the unrolled k, t >= k (the transposition's other row)
template <int N, int K>
__device__ __forceinline__ void perm_swap(double (&y)[N], int t) {
#pragma unroll
  for (int c = K + 1; c < N; c++) cswap(t == c, y[K], y[c]);
}
template <int N, int K>
__device__ __forceinline__ void perm_forward(double (&y)[N], const int (&tr)[N]) {  // P b: k = 0 .. N-1
  if constexpr (K < N) {
    perm_swap<N, K>(y, tr[K]);
    perm_forward<N, K + 1>(y, tr);
  }
}
template <int N, int K>
__device__ __forceinline__ void perm_backward(double (&y)[N], const int (&tr)[N]) {  // P^T: k = N-1 .. 0
  if constexpr (K >= 0) {
    perm_swap<N, K>(y, tr[K]);
    perm_backward<N, K - 1>(y, tr);
  }
}
template <int N>
__device__ __forceinline__ bool ldlt(const double* Hin, const double* b, double* x) {
  double m[N * N];
#pragma unroll
  for (int i = 0; i < N * N; i++) m[i] = Hin[i];
  int tr[N];
#pragma unroll
  for (int i = 0; i < N; i++) tr[i] = i;
  int sign = 0;
  bool zero = false;
  ldlt_step<N, 0>(m, tr, sign, zero);
  if (!(sign == 1 || sign == 0)) return false;
  double y[N];
#pragma unroll
  for (int i = 0; i < N; i++) y[i] = b[i];
  perm_forward<N, 0>(y, tr);
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < i; j++) y[i] -= m[N * i + j] * y[j];
  const double tol = 2.2250738585072014e-308;  // numeric_limits<double>::min()
#pragma unroll
  for (int i = 0; i < N; i++) y[i] = __builtin_fabs(m[(N + 1) * i]) > tol ? y[i] / m[(N + 1) * i] : 0.0;
#pragma unroll
  for (int i = N - 1; i >= 0; i--)
#pragma unroll
    for (int j = i + 1; j < N; j++) y[i] -= m[N * j + i] * y[j];
  perm_backward<N, N - 1>(y, tr);
#pragma unroll
  for (int i = 0; i < N; i++) x[i] = y[i];
  return true;
}

// sequential sum of m LDS values at stride st (insertion order kept), software-pipelined: the next
// 8 values load while the current 8 are added, so the chain runs at the add latency
__device__ __forceinline__ double lds_chain(const double* base, int m, int st, double s, bool sub) {
  const int m8 = m & ~7;
  double v[8];
  if (m8 > 0) {
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = base[u * st];
  }
  for (int k = 0; k < m8; k += 8) {
    double w[8];
    const int kn = k + 8 < m8 ? k + 8 : k;  // last batch: a harmless reload
#pragma unroll
    for (int u = 0; u < 8; u++) w[u] = base[(kn + u) * st];
#pragma unroll
    for (int u = 0; u < 8; u++) s = sub ? s - v[u] : s + v[u];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = w[u];
  }
  for (int k = m8; k < m; k++) s = sub ? s - base[k * st] : s + base[k * st];
  return s;
}

// ------------------------------------------------------------------------------------------------
// g2o's OptimizationAlgorithmLevenberg::solve, once: the scalar state, the start, a trial's verdict
// and the iteration-end rule.  k_pose_optimization, k_optimize_sim3 and k_eg_lm keep a Step in LDS and
// thread 0 calls these; LocalBA's k_ba_lm_control_body (ba_lm.h) runs them on a copy of its LmState's
// fields.  Host and device alike (orbx_debug_lm_step runs the host build; tests/test_lm_step.py holds
// it to the literals' lm_trial / lm_iteration_end bit for bit).
struct Step {
  double lambda, ni, currentChi, iniChi, rho;
  int qmax, nBad;
};

// optimize()'s first iteration: lambda0 is computeLambdaInit's value
__host__ __device__ __forceinline__ void start(Step& s, double lambda0) {
  s.lambda = lambda0;
  s.ni = 2;
  s.nBad = 0;
}
// computeLambdaInit without a user value: tau * max|H_jj| over an N x N row-major H
template <int N>
__host__ __device__ __forceinline__ double lambda_init(const double* H) {
  double m = 0;
  for (int j = 0; j < N; j++) {
    const double a = __builtin_fabs(H[(N + 1) * j]);
    m = (a < m) ? m : a;  // std::max(|H_jj|, m)
  }
  return 1e-5 * m;
}

// The (2 rho - 1)^3 of the accepted trial's scale factor, as each yardstick computes it.  The two are
// NOT the same function and may not be merged: they differ in the last bit for more than a quarter of
// the arguments, and each kernel equals its own yardstick bit for bit.
//   cube_product: the plain product.  oracle/poseopt.cpp (PoseOptimization), tests/optsim3_literal.py
//                 (OptimizeSim3) and tests/essgraph_literal.py (OptimizeEssentialGraph) write
//                 t3 * t3 * t3, two roundings.
//   cube_rounded: the cube rounded once.  oracle/localba.cpp (LocalBundleAdjustment) calls
//                 std::pow(x, 3) as g2o does (glibc's pow is within an ulp of it): x^2 and x^2 * x split
//                 exactly with fma, host and device alike.
enum class Cube { kProduct, kRounded };
__host__ __device__ __forceinline__ double cube_product(double x) { return x * x * x; }
__host__ __device__ __forceinline__ double cube_rounded(double x) {
  const double p = x * x, pe = __builtin_fma(x, x, -p);
  const double c = p * x, ce = __builtin_fma(p, x, -c);
  return c + (ce + pe * x);
}

struct Verdict {
  bool accept;  // the trial's state stays (else: pop)
  bool go;      // another trial of this iteration follows
};
// One trial's verdict.  tempChi: activeRobustChi2 at the trial state; scale: sum x_j (lambda x_j + b_j);
// ok2: the solve succeeded (else both are replaced, as in the reference).
template <Cube kCube>
__host__ __device__ __forceinline__ Verdict trial(Step& s, double tempChi, double scale, bool ok2) {
  if (!ok2) {
    tempChi = 1.7976931348623157e308;  // std::numeric_limits<double>::max()
    scale = 0.0;
  }
  double rho = s.currentChi - tempChi;
  scale += 1e-3;
  rho /= scale;
  const bool accept = rho > 0 && __builtin_isfinite(tempChi);
  if (accept) {
    const double t3 = 2 * rho - 1;
    double alpha = 1. - (kCube == Cube::kRounded ? cube_rounded(t3) : cube_product(t3));
    alpha = (2. / 3. < alpha) ? 2. / 3. : alpha;     // std::min(alpha, 2/3)
    s.lambda *= (1. / 3. < alpha) ? alpha : 1. / 3.;  // std::max(1/3, alpha)
    s.ni = 2;
    s.currentChi = tempChi;
  } else {
    s.lambda *= s.ni;
    s.ni *= 2;
  }
  s.qmax++;
  s.rho = rho;
  return {accept, rho < 0 && s.qmax < 10};
}
// After an iteration's last trial: true when optimize() stops (the trial budget, rho == 0, or the
// third iteration in a row that gained less than a thousandth of its starting chi)
__host__ __device__ __forceinline__ bool iteration_end(Step& s) {
  if (s.qmax == 10 || s.rho == 0) return true;
  if ((s.iniChi - s.currentChi) * 1e3 < s.iniChi) s.nBad++;
  else s.nBad = 0;
  return s.nBad >= 3;
}

// entry q of an N x N upper triangle stored row by row (c >= r): its row and column
template <int N>
__host__ __device__ __forceinline__ void tri_rc(int q, int& r, int& c) {
  r = 0;
  c = q;
  while (c >= N - r) {
    c -= N - r;
    r++;
  }
  c += r;
}

}  // namespace lm
}  // namespace orbx

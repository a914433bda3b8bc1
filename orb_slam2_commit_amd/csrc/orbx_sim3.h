// orbx_sim3.h -- g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h) on the device, shared by optsim3.hip
// (Optimizer::OptimizeSim3) and essgraph.hip (Optimizer::OptimizeEssentialGraph): the exponential
// constructor, operator*, inverse(), map(), VertexSim3Expmap::oplusImpl on a unit update, and log().
// The operation sequences are those of tests/optsim3_literal.py and tests/essgraph_literal.py;
// nothing here may be re-associated.
#pragma once
#include <hip/hip_runtime.h>

#include "orbx_device.h"
#include "orbx_lm.h"

namespace orbx {
namespace g2osim3 {

using namespace lm;

struct Sim3 {
  Quat q;
  double t[3];
  double s;
};

// Sim3(const Vector7d&), types/sim3.h:70-142
__device__ __forceinline__ Sim3 sim3_exp(const double (&u)[7]) {
  const double w[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]};
  const double sigma = u[6];
  const double theta = __builtin_sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double O[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  Sim3 T;
  T.s = exp_det(sigma);
  double O2[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) O2[3 * r + c] = O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c] + O[3 * r + 2] * O[6 + c];
  const double eps = 0.00001;
  const bool small_theta = theta < eps;
  double sn = 0, cs = 0, ra = 1.0, rb = 1.0;  // R = I + ra*Omega + rb*Omega2 (both 1: the products are skipped)
  if (!small_theta) {
    sincos_d(theta, &sn, &cs);
    ra = sn / theta;
    rb = (1 - cs) / (theta * theta);
  }
  double A, B, C;
  if (__builtin_fabs(sigma) < eps) {
    C = 1;
    if (small_theta) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cs) / (theta2);
      B = (theta - sn) / (theta2 * theta);
    }
  } else {
    C = (T.s - 1) / sigma;
    if (small_theta) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * T.s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * T.s) / (sigma2 * sigma);
    } else {
      const double a = T.s * sn;
      const double b = T.s * cs;
      const double theta2 = theta * theta;
      const double sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  double R[9], W[9];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const double I = (i % 4) == 0 ? 1.0 : 0.0;
    R[i] = small_theta ? I + O[i] + O2[i] : I + ra * O[i] + rb * O2[i];
    W[i] = A * O[i] + B * O2[i] + C * I;
  }
  T.q = mat2q(R);  // Quaterniond(R): Sim3 never normalises
#pragma unroll
  for (int r = 0; r < 3; r++) T.t[r] = W[3 * r] * up[0] + W[3 * r + 1] * up[1] + W[3 * r + 2] * up[2];
  return T;
}
// operator*, sim3.h:266-272
__device__ __forceinline__ Sim3 sim3_mul(const Sim3& a, const Sim3& b) {
  Sim3 r;
  double rt[3];
  qrot(a.q, b.t, rt);
  r.q = qmul(a.q, b.q);
#pragma unroll
  for (int i = 0; i < 3; i++) r.t[i] = a.s * rt[i] + a.t[i];
  r.s = a.s * b.s;
  return r;
}
// inverse(), sim3.h:233-236
__device__ __forceinline__ Sim3 sim3_inverse(const Sim3& S) {
  Sim3 r;
  r.q.x = -S.q.x; r.q.y = -S.q.y; r.q.z = -S.q.z; r.q.w = S.q.w;
  const double c = -1. / S.s;
  const double v[3] = {c * S.t[0], c * S.t[1], c * S.t[2]};
  qrot(r.q, v, r.t);
  r.s = 1. / S.s;
  return r;
}
// VertexSim3Expmap::oplusImpl with the update e_d * step (d in 0..6; d < 0: the zero update)
__device__ __forceinline__ Sim3 oplus_unit(const Sim3& S, int d, double step, bool fix_scale) {
  double u[7];
#pragma unroll
  for (int k = 0; k < 7; k++) u[k] = k == d ? step : 0.0;
  if (fix_scale) u[6] = 0;
  return sim3_mul(sim3_exp(u), S);
}
// map(), sim3.h:144-146
__device__ __forceinline__ void sim3_map(const Sim3& S, const double X[3], double out[3]) {
  double r[3];
  qrot(S.q, X, r);
#pragma unroll
  for (int i = 0; i < 3; i++) out[i] = S.s * r[i] + S.t[i];
}
__device__ __forceinline__ Sim3 sim3_load(const double* v) {
  Sim3 S;
  S.q.x = v[0]; S.q.y = v[1]; S.q.z = v[2]; S.q.w = v[3];
  S.t[0] = v[4]; S.t[1] = v[5]; S.t[2] = v[6];
  S.s = v[7];
  return S;
}
__device__ __forceinline__ void sim3_store(const Sim3& S, double* v) {
  v[0] = S.q.x; v[1] = S.q.y; v[2] = S.q.z; v[3] = S.q.w;
  v[4] = S.t[0]; v[5] = S.t[1]; v[6] = S.t[2];
  v[7] = S.s;
}

// log(), sim3.h:148-230.  std::log and acos are log_det / acos_det, sin and cos are sincos_d.
// W = (A*Omega + (B*Omega)*Omega) + C*I; W.lu().solve(t) is Eigen's PartialPivLU at 3x3 (first
// largest |entry| of the column pivots, the column below is divided by the pivot, the trailing block
// takes the outer product) followed by its two column-oriented triangular solves.  The row exchanges
// are value selects on named entries (orbx_lm.h: a run-time index would move W to scratch memory).
// *branch (optional): bit 0 = the d <= 1 - eps side, bit 1 = the |sigma| >= eps side, bit 2 = a row
// exchange at the first pivot, bit 3 = at the second.
__device__ __forceinline__ void sim3_log(const Sim3& S, double (&res)[7], int* branch = nullptr) {
  const double sigma = log_det(S.s);
  double R[9];
  qmat(S.q, R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double eps = 0.00001;
  const bool small_sigma = __builtin_fabs(sigma) < eps;
  const bool small_rot = d > 1 - eps;
  double om[3], theta = 0, sn = 0, cs = 0;
  if (small_rot) {
#pragma unroll
    for (int i = 0; i < 3; i++) om[i] = 0.5 * dR[i];
  } else {
    theta = acos_det(d);
    const double f = theta / (2 * __builtin_sqrt(1 - d * d));
#pragma unroll
    for (int i = 0; i < 3; i++) om[i] = f * dR[i];
    sincos_d(theta, &sn, &cs);
  }
  double A, B, C;
  if (small_sigma) {
    C = 1;
    if (small_rot) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cs) / (theta2);
      B = (theta - sn) / (theta2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (small_rot) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * S.s + 1) / (sigma2);
      B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
    } else {
      const double theta2 = theta * theta;
      const double a = S.s * sn;
      const double b = S.s * cs;
      const double c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
  double BO[9], W[9];
#pragma unroll
  for (int i = 0; i < 9; i++) BO[i] = B * O[i];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double I = r == c ? 1.0 : 0.0;
      const double p = BO[3 * r] * O[c] + BO[3 * r + 1] * O[3 + c] + BO[3 * r + 2] * O[6 + c];
      W[3 * r + c] = A * O[3 * r + c] + p + C * I;
    }
  double y[3] = {S.t[0], S.t[1], S.t[2]};
  int br = (small_rot ? 0 : 1) | (small_sigma ? 0 : 2);
  {  // pivot 0
    int big = 0;
    double bv = __builtin_fabs(W[0]);
    if (__builtin_fabs(W[3]) > bv) { bv = __builtin_fabs(W[3]); big = 1; }
    if (__builtin_fabs(W[6]) > bv) { bv = __builtin_fabs(W[6]); big = 2; }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      cswap(big == 1, W[c], W[3 + c]);
      cswap(big == 2, W[c], W[6 + c]);
    }
    cswap(big == 1, y[0], y[1]);
    cswap(big == 2, y[0], y[2]);
    if (big != 0) br |= 4;
    if (bv != 0.0) {
      W[3] /= W[0];
      W[6] /= W[0];
    }
    W[4] -= W[3] * W[1]; W[5] -= W[3] * W[2];
    W[7] -= W[6] * W[1]; W[8] -= W[6] * W[2];
  }
  {  // pivot 1
    const bool sw = __builtin_fabs(W[7]) > __builtin_fabs(W[4]);
#pragma unroll
    for (int c = 0; c < 3; c++) cswap(sw, W[3 + c], W[6 + c]);
    cswap(sw, y[1], y[2]);
    if (sw) br |= 8;
    if (W[4] != 0.0) W[7] /= W[4];
    W[8] -= W[7] * W[5];
  }
  // L (unit lower), column by column
  y[1] -= y[0] * W[3];
  y[2] -= y[0] * W[6];
  y[2] -= y[1] * W[7];
  // U, column by column from the last
  y[2] /= W[8];
  y[0] -= y[2] * W[2];
  y[1] -= y[2] * W[5];
  y[1] /= W[4];
  y[0] -= y[1] * W[1];
  y[0] /= W[0];
  res[0] = om[0]; res[1] = om[1]; res[2] = om[2];
  res[3] = y[0]; res[4] = y[1]; res[5] = y[2];
  res[6] = sigma;
  if (branch) *branch = br;
}

}  // namespace g2osim3
}  // namespace orbx

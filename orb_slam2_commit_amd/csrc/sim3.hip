// sim3.hip -- Sim3Solver (src/Sim3Solver.cc:37-481) on the GPU: the RANSAC stage of
// LoopClosing::ComputeSim3 (src/LoopClosing.cc:372-402).
//
//   k_sim3_hyp     one 256-thread block per (hypothesis, solver): ComputeSim3 (:264-393, Horn 1987 on
//                  the 3 sampled pairs) on lane 0 with the 4x4 Jacobi's matrices in LDS, then
//                  CheckInliers (:396-422) of every correspondence by all threads -> mask + count
//   k_sim3_select  one wave per solver: the walk of iterate() (:174-232) over the counts in
//                  iteration order (`>=` replaces the best, the first replacement above
//                  mRansacMinInliers returns), the winner copied into the solver's device-resident
//                  best state, mnIterations advanced, one result record (+ the returned mask)
// Every iteration draws exactly 3 values and a solver that returns nothing runs all of its
// iterations, so the minimal sets of a call are replayed on the host from the rand() values
// (DUtils::Random::RandomInt + swap-remove) before anything is launched: one upload (job records
// + sets), two launches, one readback per call, for one solver or many.
//
// Arithmetic: the OpenCV 3.2 calls of ComputeSim3 restated operation by operation (DESIGN.md,
// parity: cv::reduce, the transposed gemm, JacobiImpl_<float>, cv::norm, the MatExpr scalings,
// cv::Rodrigues, the small-matrix gemm, Mat::dot), float and double exactly where the library uses
// them, -ffp-contract=off; atan2 / sin / cos through atan2_det / sincos_d.  tests/sim3_literal.py
// is the same sequence in numpy scalars, and the GPU equals it bit for bit.
//
// Bound: latency.  A block's life is the serial Horn solve on one lane (a few tens of dependent
// Jacobi rotations); the check reads 48 B and writes 1 B per correspondence, N in the hundreds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/orbx.h"
#include "../../include/orbx_debug.h"
#include "orbx_cv.h"
#include "orbx_device.h"
#include "orbx_ransac.h"

namespace orbx {

struct Sim3In {
  const float* x1;   // mvX3Dc1, N x 3
  const float* x2;   // mvX3Dc2, N x 3
  const float* p1;   // mvP1im1, N x 2
  const float* p2;   // mvP2im2, N x 2
  const float* me1;  // (float)mvnMaxError1, N
  const float* me2;
  int N, fix_scale;
  float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
};

struct Sim3Hyp {  // one hypothesis / the best so far: mT12i, mR12i, mt12i, ms12i
  float T12[16];
  float R[9];
  float t[3];
  float s;
  float pad[3];
};
static_assert(sizeof(Sim3Hyp) == 128, "Sim3Hyp");

struct Sim3State {  // device-resident solver state
  int iterations;   // mnIterations
  int best_inliers; // mnBestInliers
  int pad[2];
  Sim3Hyp best;     // mBestT12, mBestRotation, mBestTranslation, mBestScale
};

struct Sim3Rec {  // result record of one iterate() call
  int no_more, found, n_inliers, done;  // done: iterations this call ran
  int iterations, best_inliers, pad[2];
  float T12[16];
};
static_assert(sizeof(Sim3Rec) == 96, "Sim3Rec");

struct Sim3Job {
  Sim3In in;
  const int* sets;  // H x 3 indices
  Sim3Hyp* hyps;    // H
  uint8_t* masks;   // H x N
  int* counts;      // H
  Sim3State* state;
  uint8_t* best_mask;  // N, mvbBestInliers
  Sim3Rec* rec;
  uint8_t* out_mask;   // N, written when found
  int H;               // iterations this call may run: min(nIterations, mRansacMaxIts - mnIterations)
  int max_its, min_inliers;
  int too_few;         // N < mRansacMinInliers: bNoMore, nothing else
};

// ------------------------------------------------------------------ ComputeSim3
// hypot of OpenCV's lapack.cpp (float)
__device__ __forceinline__ float cv_hypot(float a, float b) {
  a = __builtin_fabsf(a);
  b = __builtin_fabsf(b);
  if (a > b) {
    b /= a;
    return a * __builtin_sqrtf(1 + b * b);
  }
  if (b > 0) {
    a /= b;
    return b * __builtin_sqrtf(1 + a * a);
  }
  return 0;
}

// JacobiImpl_<float> (cv::eigen on a 4x4 CV_32F): A, V (4x4, row stride 4), W (4), ind (indR | indC)
// in LDS because the pivot indices are run-time values.  On return row 0 of V is the eigenvector
// of the largest eigenvalue.
__device__ void jacobi4(float* A, float* W, float* V, int* ind) {
  const int n = 4;
  const float eps = 1.1920928955078125e-07f;  // FLT_EPSILON
  int* indR = ind;
  int* indC = ind + n;
  int i, j, k, m;
  for (i = 0; i < n; i++) {
    for (j = 0; j < n; j++) V[i * 4 + j] = 0.f;
    V[i * 4 + i] = 1.f;
  }
  float mv = 0.f;
  for (k = 0; k < n; k++) {
    W[k] = A[5 * k];
    if (k < n - 1) {
      for (m = k + 1, mv = __builtin_fabsf(A[4 * k + m]), i = k + 2; i < n; i++) {
        const float val = __builtin_fabsf(A[4 * k + i]);
        if (mv < val) mv = val, m = i;
      }
      indR[k] = m;
    }
    if (k > 0) {
      for (m = 0, mv = __builtin_fabsf(A[k]), i = 1; i < k; i++) {
        const float val = __builtin_fabsf(A[4 * i + k]);
        if (mv < val) mv = val, m = i;
      }
      indC[k] = m;
    }
  }
  const int maxIters = n * n * 30;
  for (int iters = 0; iters < maxIters; iters++) {
    for (k = 0, mv = __builtin_fabsf(A[indR[0]]), i = 1; i < n - 1; i++) {
      const float val = __builtin_fabsf(A[4 * i + indR[i]]);
      if (mv < val) mv = val, k = i;
    }
    int l = indR[k];
    for (i = 1; i < n; i++) {
      const float val = __builtin_fabsf(A[4 * indC[i] + i]);
      if (mv < val) mv = val, k = indC[i], l = i;
    }
    const float p = A[4 * k + l];
    if (__builtin_fabsf(p) <= eps) break;
    const float y = (float)((double)(W[l] - W[k]) * 0.5);
    float t = __builtin_fabsf(y) + cv_hypot(p, y);
    float s = cv_hypot(p, t);
    const float c = t / s;
    s = p / s;
    t = (p / t) * p;
    if (y < 0) s = -s, t = -t;
    A[4 * k + l] = 0;
    W[k] -= t;
    W[l] += t;
    float a0, b0;
#define ORBX_ROT(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
    for (i = 0; i < k; i++) ORBX_ROT(A[4 * i + k], A[4 * i + l]);
    for (i = k + 1; i < l; i++) ORBX_ROT(A[4 * k + i], A[4 * i + l]);
    for (i = l + 1; i < n; i++) ORBX_ROT(A[4 * k + i], A[4 * l + i]);
    for (i = 0; i < n; i++) ORBX_ROT(V[4 * k + i], V[4 * l + i]);
#undef ORBX_ROT
    for (j = 0; j < 2; j++) {
      const int idx = j == 0 ? k : l;
      if (idx < n - 1) {
        for (m = idx + 1, mv = __builtin_fabsf(A[4 * idx + m]), i = idx + 2; i < n; i++) {
          const float val = __builtin_fabsf(A[4 * idx + i]);
          if (mv < val) mv = val, m = i;
        }
        indR[idx] = m;
      }
      if (idx > 0) {
        for (m = 0, mv = __builtin_fabsf(A[idx]), i = 1; i < idx; i++) {
          const float val = __builtin_fabsf(A[4 * i + idx]);
          if (mv < val) mv = val, m = i;
        }
        indC[idx] = m;
      }
    }
  }
  // eigenvalues descending, rows of V with them
  for (k = 0; k < n - 1; k++) {
    m = k;
    for (i = k + 1; i < n; i++)
      if (W[m] < W[i]) m = i;
    if (k != m) {
      const float w = W[m];
      W[m] = W[k];
      W[k] = w;
      for (i = 0; i < n; i++) {
        const float v = V[4 * m + i];
        V[4 * m + i] = V[4 * k + i];
        V[4 * k + i] = v;
      }
    }
  }
}

// ComputeCentroid (:247-262): cv::reduce(SUM) over a 3-column row is (p0 + p2) + p1 (reduceC_'s
// two accumulators), C/3 is convertTo(1./3), then Pr = P - C.  P, Pr: 3x3, one point per column.
__device__ __forceinline__ void sim3_centroid(const float P[9], float Pr[9], float C[3]) {
  const float third = (float)(1. / 3);
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float sum = (P[3 * r] + P[3 * r + 2]) + P[3 * r + 1];
    C[r] = sum * third + 0.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) Pr[3 * r + c] = P[3 * r + c] - C[r];
  }
}

// ComputeSim3 (:264-393) of the pairs `idx`; out: the hypothesis record, T (LDS): T12 rows 0-2
// (12 floats) then T21 rows 0-2.  sA/sV/sW/sInd: the Jacobi's LDS.
__device__ void sim3_compute(const Sim3In& in, const int* __restrict__ idx, float* sA, float* sV, float* sW,
                             int* sInd, Sim3Hyp* __restrict__ out, float* __restrict__ T) {
  float P1[9], P2[9];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int i = idx[c];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      P1[3 * r + c] = in.x1[3 * i + r];
      P2[3 * r + c] = in.x2[3 * i + r];
    }
  }
  // Step 1
  float Pr1[9], Pr2[9], O1[3], O2[3];
  sim3_centroid(P1, Pr1, O1);
  sim3_centroid(P2, Pr2, O2);
  // Step 2: M = Pr2 * Pr1.t(), GEMMSingleMul<float,double>: the sum in double, rounded once
  float M[9];
  cvmat::gemm33_bt<3>(Pr2, Pr1, 1.0, M);
  // Step 3: N (float sums, left to right)
  const float N11 = M[0] + M[4] + M[8], N12 = M[5] - M[7], N13 = M[6] - M[2], N14 = M[1] - M[3];
  const float N22 = M[0] - M[4] - M[8], N23 = M[1] + M[3], N24 = M[6] + M[2];
  const float N33 = -M[0] + M[4] - M[8], N34 = M[5] + M[7], N44 = -M[0] - M[4] + M[8];
  sA[0] = N11, sA[1] = N12, sA[2] = N13, sA[3] = N14;
  sA[4] = N12, sA[5] = N22, sA[6] = N23, sA[7] = N24;
  sA[8] = N13, sA[9] = N23, sA[10] = N33, sA[11] = N34;
  sA[12] = N14, sA[13] = N24, sA[14] = N34, sA[15] = N44;
  // Step 4
  jacobi4(sA, sW, sV, sInd);
  const float q0 = sV[0];
  float vec[3] = {sV[1], sV[2], sV[3]};
  const double nrm = cvmat::norm3(vec);
  const double ang = atan2_det(nrm, (double)q0);
  // vec = 2*ang*vec/norm(vec): one MatExpr scale alpha = (2*ang) * (1./norm), convertTo (always the product)
#pragma unroll
  for (int i = 0; i < 3; i++) vec[i] = cvmat::scale<false>(vec[i], (2 * ang) * (1. / nrm));
  // cv::Rodrigues
  float R[9];
  {
    double rx = vec[0], ry = vec[1], rz = vec[2];
    const double theta = __builtin_sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < 2.2204460492503131e-16) {
#pragma unroll
      for (int k = 0; k < 9; k++) R[k] = (k % 4) == 0 ? 1.f : 0.f;
    } else {
      double s, c;
      sincos_d(theta, &s, &c);
      const double c1 = 1. - c;
      const double itheta = theta ? 1. / theta : 0.;
      rx *= itheta;
      ry *= itheta;
      rz *= itheta;
      const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
      const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
#pragma unroll
      for (int k = 0; k < 9; k++) R[k] = (float)(c * ((k % 4) == 0 ? 1. : 0.) + c1 * rrt[k] + s * r_x[k]);
    }
  }
  // Step 5: P3 = R * Pr2
  float P3[9];
  cvmat::gemm33<3>(R, Pr2, 1.0, P3);
  // Step 6
  float s12;
  if (!in.fix_scale) {
    const double nom = cvmat::dot<9>(Pr1, P3);  // (two sums of four, then the tail)
    double den = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) den += (double)(P3[k] * P3[k]);
    s12 = (float)(nom / den);
  } else {
    s12 = 1.0f;
  }
  // Step 7: t12 = O1 - s*R*O2, one gemm with alpha = -s, beta = 1
  float t12[3];
  cvmat::gemm31_add<3>(R, O2, -(double)s12, O1, t12);
  // Step 8.1: T12 = [s*R | t12] (always the product)
  float sR[9];
#pragma unroll
  for (int k = 0; k < 9; k++) sR[k] = cvmat::scale<false>(R[k], (double)s12);
  // Step 8.2: T21 = [(1/s)*R.t() | -sRinv*t12]; the transpose alone when the scale is exactly 1
  const double ia = 1.0 / (double)s12;
  float sRinv[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) sRinv[3 * i + j] = ia != 1.0 ? cvmat::scale<false>(R[3 * j + i], ia) : R[3 * j + i];
  float tinv[3];
  cvmat::gemm31<3>(sRinv, t12, -1.0, tinv);
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      T[4 * r + c] = sR[3 * r + c];
      T[12 + 4 * r + c] = sRinv[3 * r + c];
      out->T12[4 * r + c] = sR[3 * r + c];
    }
    T[4 * r + 3] = t12[r];
    T[12 + 4 * r + 3] = tinv[r];
    out->T12[4 * r + 3] = t12[r];
    out->t[r] = t12[r];
  }
  out->T12[12] = 0.f, out->T12[13] = 0.f, out->T12[14] = 0.f, out->T12[15] = 1.f;
#pragma unroll
  for (int k = 0; k < 9; k++) out->R[k] = R[k];
  out->s = s12;
}

// Project (:440-461) of one point: R*X + t is the small-matrix gemm (float sum, the addition in
// double rounded to float), then the pinhole in float.
__device__ __forceinline__ void sim3_project(const float* __restrict__ T, const float X[3], float fx, float fy,
                                             float cx, float cy, float* u, float* v) {
  float P[3];
  cvmat::pose_apply(T, X, P);
  const float invz = 1 / P[2];
  const float x = P[0] * invz, y = P[1] * invz;
  *u = fx * x + cx;
  *v = fy * y + cy;
}

struct Sim3Corr {
  float x1[3], x2[3], p1[2], p2[2], me1, me2;
};
__device__ __forceinline__ Sim3Corr sim3_load(const Sim3In& in, int i) {
  Sim3Corr c;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c.x1[k] = in.x1[3 * i + k];
    c.x2[k] = in.x2[3 * i + k];
  }
  c.p1[0] = in.p1[2 * i], c.p1[1] = in.p1[2 * i + 1];
  c.p2[0] = in.p2[2 * i], c.p2[1] = in.p2[2 * i + 1];
  c.me1 = in.me1[i];
  c.me2 = in.me2[i];
  return c;
}
// CheckInliers (:396-422) of one correspondence; a NaN error is no inlier
__device__ __forceinline__ bool sim3_inlier(const Sim3In& in, const float* __restrict__ T, const Sim3Corr& c) {
  float u, v;
  sim3_project(T, c.x2, in.fx1, in.fy1, in.cx1, in.cy1, &u, &v);  // vP2im1
  const float d10 = c.p1[0] - u, d11 = c.p1[1] - v;
  sim3_project(T + 12, c.x1, in.fx2, in.fy2, in.cx2, in.cy2, &u, &v);  // vP1im2
  const float d20 = u - c.p2[0], d21 = v - c.p2[1];
  const float err1 = (float)((double)d10 * (double)d10 + (double)d11 * (double)d11);
  const float err2 = (float)((double)d20 * (double)d20 + (double)d21 * (double)d21);
  return err1 < c.me1 && err2 < c.me2;
}

constexpr int kSim3Threads = 256;

__global__ __launch_bounds__(kSim3Threads) void k_sim3_hyp(const Sim3Job* __restrict__ jobs) {
  const Sim3Job& J = jobs[blockIdx.y];
  if ((int)blockIdx.x >= J.H) return;  // block-uniform
  __shared__ float sA[16], sV[16], sW[4], sT[24];
  __shared__ int sInd[8], red[kSim3Threads / 64];
  const int h = blockIdx.x, tid = threadIdx.x, N = J.in.N;
  // the first correspondence of every thread is fetched while lane 0 solves
  Sim3Corr c0;
  if (tid < N) c0 = sim3_load(J.in, tid);
  if (tid == 0) sim3_compute(J.in, J.sets + 3 * (size_t)h, sA, sV, sW, sInd, J.hyps + h, sT);
  __syncthreads();
  uint8_t* __restrict__ m = J.masks + (size_t)h * N;
  int cnt = 0;
  if (tid < N) {
    const bool ok = sim3_inlier(J.in, sT, c0);
    m[tid] = ok;
    cnt += ok;
  }
  for (int i = tid + kSim3Threads; i < N; i += kSim3Threads) {
    const bool ok = sim3_inlier(J.in, sT, sim3_load(J.in, i));
    m[i] = ok;
    cnt += ok;
  }
  cnt = wave_sum(cnt);
  if ((tid & 63) == 0) red[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) J.counts[h] = red[0] + red[1] + red[2] + red[3];
}

// ------------------------------------------------------------------ the walk
struct Sim3Pick {
  int found;  // iteration that returned, -1: none
  int bestk;  // last iteration that replaced the best, -1: none
  int best;   // mnBestInliers afterwards
};

// iterate()'s loop (:174-232) over the counts of one solver, one wave: iteration k replaces the
// best iff counts[k] >= every earlier count and the carried-over best (an inclusive prefix
// maximum), and returns iff it replaced and counts[k] > mRansacMinInliers.
__device__ __forceinline__ Sim3Pick sim3_walk(const Sim3Job& J, int lane) {
  Sim3Pick p{-1, -1, J.state->best_inliers};
  if (J.too_few) return p;
  for (int base = 0; base < J.H; base += 64) {
    const int k = base + lane;
    const int c = k < J.H ? J.counts[k] : -1;
    int m = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(m, o, 64);
      if (lane >= o) m = max(m, v);
    }
    const int incl = max(m, p.best);
    const bool repl = k < J.H && c == incl;
    const bool ret = repl && c > J.min_inliers;
    const unsigned long long rb = __ballot(ret), pb = __ballot(repl);
    if (rb) {
      const int f = __builtin_ctzll(rb);
      p.found = p.bestk = base + f;
      p.best = __shfl(c, f, 64);
      break;
    }
    if (pb) p.bestk = base + 63 - __builtin_clzll(pb);
    p.best = __shfl(incl, 63, 64);
  }
  return p;
}

__device__ __forceinline__ void sim3_commit(const Sim3Job& J, const Sim3Pick& p, int lane) {
  Sim3Rec* __restrict__ rec = J.rec;
  if (J.too_few) {
    if (lane < 24) ((int*)rec)[lane] = lane == 0 ? 1 : 0;
    return;
  }
  const int N = J.in.N;
  const int done = p.found >= 0 ? p.found + 1 : J.H;
  const int its = J.state->iterations + done;
  if (p.bestk >= 0) {
    const float* src = (const float*)(J.hyps + p.bestk);
    if (lane < 32) ((float*)&J.state->best)[lane] = src[lane];
    const uint8_t* ms = J.masks + (size_t)p.bestk * N;
    for (int i = lane; i < N; i += 64) J.best_mask[i] = ms[i];
  }
  if (p.found >= 0) {
    const uint8_t* ms = J.masks + (size_t)p.found * N;
    for (int i = lane; i < N; i += 64) J.out_mask[i] = ms[i];
    if (lane < 16) rec->T12[lane] = J.hyps[p.found].T12[lane];
  } else if (lane < 16) {
    rec->T12[lane] = 0.f;
  }
  if (lane == 0) {
    J.state->iterations = its;
    J.state->best_inliers = p.best;
    rec->no_more = p.found < 0 && its >= J.max_its;
    rec->found = p.found >= 0;
    rec->n_inliers = p.found >= 0 ? p.best : 0;
    rec->done = done;
    rec->iterations = its;
    rec->best_inliers = p.best;
    rec->pad[0] = rec->pad[1] = 0;
  }
}

// shared = 0: grid = solvers, one wave each, independent.  shared = 1 (the candidate sweep of
// LoopClosing, :372-402): one block, a wave per solver, up to 16 at a time in order; a solver
// commits only when no earlier one returned (decided through LDS, never through global atomics),
// the ones after the first that returned are left untouched.
__global__ __launch_bounds__(1024) void k_sim3_select(const Sim3Job* __restrict__ jobs, int n, int shared) {
  __shared__ int s_found[16];
  const int W = blockDim.x >> 6, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (!shared) {
    const Sim3Job& J = jobs[blockIdx.x];
    sim3_commit(J, sim3_walk(J, lane), lane);
    return;
  }
  for (int base = 0; base < n; base += W) {
    const int s = base + w;
    Sim3Pick p{-1, -1, 0};
    if (s < n) p = sim3_walk(jobs[s], lane);
    if (lane == 0) s_found[w] = s < n && p.found >= 0;
    __syncthreads();
    bool earlier = false, any = false;
    for (int j = 0; j < W; j++) {
      any |= s_found[j] != 0;
      earlier |= j < w && s_found[j] != 0;
    }
    if (s < n && !earlier) sim3_commit(jobs[s], p, lane);
    __syncthreads();
    if (any) break;  // block-uniform
  }
}

struct Sim3GatherJob {
  const uint8_t* src;
  uint8_t* dst;
  int bytes;  // multiple of 16
};
__global__ __launch_bounds__(256) void k_sim3_gather(const Sim3GatherJob* __restrict__ jobs) {
  const Sim3GatherJob J = jobs[blockIdx.x];
  const uint4* s = (const uint4*)J.src;
  uint4* d = (uint4*)J.dst;
  for (int i = threadIdx.x; i < J.bytes / 16; i += 256) d[i] = s[i];
}

}  // namespace orbx

// ------------------------------------------------------------------ host / C ABI
namespace {

using orbx::Sim3GatherJob;
using orbx::Sim3Hyp;
using orbx::Sim3In;
using orbx::Sim3Job;
using orbx::Sim3Rec;
using orbx::Sim3State;

// One context per device (orbx_ransac.h), shared by every solver (LoopClosing creates a Sim3Solver
// per loop candidate): a solver owns only its correspondences, its best mask and its state; the
// per-hypothesis arrays of a call live in the context's device staging block.
orbx::RansacDevice* const g_sim3_dev = new orbx::RansacDevice[64];  // never deleted (orbx_mem.h)

}  // namespace

struct orbx_sim3 {
  int device = 0;
  hipStream_t st = nullptr;
  int N = 0, fix_scale = 0;
  float K1[4], K2[4];
  double prob = 0.99;
  int min_inliers = 6, max_its = 300;
  // host mirrors of the device state (refreshed from every result record)
  int iterations = 0, best_inliers = 0;
  // device (one allocation): x1 | x2 | p1 | p2 | me1 | me2 | best mask | state
  uint8_t* d_mem = nullptr;
  float *d_x1 = nullptr, *d_x2 = nullptr, *d_p1 = nullptr, *d_p2 = nullptr, *d_me1 = nullptr, *d_me2 = nullptr;
  uint8_t* d_best = nullptr;
  Sim3State* d_state = nullptr;
  size_t layout(uint8_t* base) {
    const size_t nn = std::max(N, 1);
    size_t o = 0;
    auto take = [&](size_t bytes) {
      uint8_t* p = base ? base + o : nullptr;
      o += orbx::scratch_align(bytes);
      return p;
    };
    d_x1 = (float*)take(12 * nn);
    d_x2 = (float*)take(12 * nn);
    d_p1 = (float*)take(8 * nn);
    d_p2 = (float*)take(8 * nn);
    d_me1 = (float*)take(4 * nn);
    d_me2 = (float*)take(4 * nn);
    d_best = take(nn);
    d_state = (Sim3State*)take(sizeof(Sim3State));
    return o;
  }
  size_t upload_bytes() const { return (size_t)((uint8_t*)d_best - (uint8_t*)d_x1); }  // the correspondences
  Sim3In in() const {
    return Sim3In{d_x1, d_x2, d_p1, d_p2, d_me1, d_me2, N, fix_scale, K1[0], K1[1], K1[2], K1[3],
                  K2[0], K2[1], K2[2], K2[3]};
  }
};

namespace {

// SetRansacParameters (src/Sim3Solver.cc:127-151); false: N < 3 with N >= minInliers, where the
// reference samples 3 of fewer than 3 (undefined)
bool sim3_derive(int N, const orbx_sim3_params* prm, int* max_its) {
  if (N >= prm->min_inliers && N < 3) return false;
  const float epsilon = (float)prm->min_inliers / N;
  int nIterations;
  if (prm->min_inliers == N) {
    nIterations = 1;
  } else {
    const double v = std::ceil(std::log(1 - prm->probability) / std::log(1 - std::pow(epsilon, 3)));
    // the double -> int conversion of the reference's x86 build: out of range and NaN give INT_MIN
    nIterations = (v == v && v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN;
  }
  *max_its = std::max(1, std::min(nIterations, prm->max_iterations));
  return true;
}

orbx_status sim3_check_problem(const orbx_sim3_solver_problem* p, const orbx_sim3_params* prm) {
  if (!p || !prm || p->n < 0) return ORBX_ERR_ARG;
  if (p->n > 0 && (!p->x3dc1 || !p->x3dc2 || !p->sigma2_1 || !p->sigma2_2)) return ORBX_ERR_ARG;
  int its;
  if (!sim3_derive(p->n, prm, &its)) return ORBX_ERR_ARG;
  return ORBX_OK;
}

orbx_sim3* sim3_new(const orbx_sim3_solver_problem* p, const orbx_sim3_params* prm, int device) {
  orbx_sim3* h = new (std::nothrow) orbx_sim3();
  if (!h) return nullptr;
  h->device = device;
  h->st = g_sim3_dev[device].st;
  h->N = p->n;
  h->fix_scale = p->fix_scale != 0;
  h->K1[0] = p->fx1, h->K1[1] = p->fy1, h->K1[2] = p->cx1, h->K1[3] = p->cy1;
  h->K2[0] = p->fx2, h->K2[1] = p->fy2, h->K2[2] = p->cx2, h->K2[3] = p->cy2;
  h->prob = prm->probability;
  h->min_inliers = prm->min_inliers;
  (void)sim3_derive(h->N, prm, &h->max_its);
  return h;
}

// The constructor's derived arrays (:95-96, :121-122) laid out as in the solver's device block:
// mvnMaxError = 9.210 * sigma2 in double truncated to size_t (compared as float), and
// FromCameraToImage (:463-481) of both point sets.
void sim3_stage(const orbx_sim3* h, const orbx_sim3_solver_problem* p, uint8_t* dst) {
  const int n = p->n;
  const uint8_t* base = (const uint8_t*)h->d_x1;
  auto at = [&](const void* d) { return (float*)(dst + ((const uint8_t*)d - base)); };
  std::memcpy(at(h->d_x1), p->x3dc1, 12 * (size_t)n);
  std::memcpy(at(h->d_x2), p->x3dc2, 12 * (size_t)n);
  float *p1 = at(h->d_p1), *p2 = at(h->d_p2), *me1 = at(h->d_me1), *me2 = at(h->d_me2);
  for (int i = 0; i < n; i++) {
    for (int side = 0; side < 2; side++) {
      const float* X = (side ? p->x3dc2 : p->x3dc1) + 3 * i;
      const float* K = side ? h->K2 : h->K1;
      const float invz = 1 / X[2];
      const float x = X[0] * invz, y = X[1] * invz;
      float* o = (side ? p2 : p1) + 2 * i;
      o[0] = K[0] * x + K[2];
      o[1] = K[1] * y + K[3];
    }
    me1[i] = (float)(size_t)(9.210 * p->sigma2_1[i]);
    me2[i] = (float)(size_t)(9.210 * p->sigma2_2[i]);
  }
}

orbx_status sim3_alloc(orbx_sim3* h) {
  const size_t bytes = h->layout(nullptr);
  if (hipMallocAsync((void**)&h->d_mem, bytes, h->st) != hipSuccess) return ORBX_ERR_HIP;
  h->layout(h->d_mem);
  // mnIterations = mnBestInliers = 0, empty best
  if (hipMemsetAsync(h->d_best, 0, bytes - (size_t)(h->d_best - h->d_mem), h->st) != hipSuccess) return ORBX_ERR_HIP;
  return ORBX_OK;
}

void sim3_free(orbx_sim3* h) {
  if (!h) return;
  if (h->d_mem) (void)hipFreeAsync(h->d_mem, h->st);
  delete h;
}

struct Sim3Run {
  orbx_sim3* h = nullptr;
  const int32_t* rv = nullptr;  // the 3 * H rand() values this call may consume
  int H = 0;
  bool too_few = false;
  Sim3Rec rec;
};

// iterations a call may run: while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations)
void sim3_begin(Sim3Run& r, int n_iterations) {
  const orbx_sim3* h = r.h;
  r.too_few = h->N < h->min_inliers;
  r.H = r.too_few ? 0 : std::max(0, std::min(n_iterations, h->max_its - h->iterations));
}

// One call for `runs`: upload (jobs + minimal sets), k_sim3_hyp over every (hypothesis, solver),
// k_sim3_select, one readback (records + returned masks).  shared: the candidate sweep.
orbx_status sim3_run(std::vector<Sim3Run>& runs, bool shared, uint8_t* const* inliers) {
  const int n = (int)runs.size();
  const int device = runs[0].h->device;
  orbx::RansacDevice& dev = g_sim3_dev[device];
  hipStream_t st = dev.st;
  // staging layout: [jobs | sets] uploaded, [hyps | masks | counts] device only, [recs + masks] read back
  const size_t off_sets = orbx::scratch_align(sizeof(Sim3Job) * (size_t)n);
  size_t o = off_sets;
  std::vector<size_t> o_sets(n), o_hyps(n), o_masks(n), o_counts(n), o_rec(n);
  int Hmax = 0;
  for (int i = 0; i < n; i++) {
    o_sets[i] = o;
    o += orbx::scratch_align(sizeof(int) * 3 * (size_t)runs[i].H);
    Hmax = std::max(Hmax, runs[i].H);
  }
  const size_t up_bytes = o;
  for (int i = 0; i < n; i++) {
    const size_t H = runs[i].H, N = std::max(runs[i].h->N, 1);
    o_hyps[i] = o;
    o += orbx::scratch_align(sizeof(Sim3Hyp) * H);
    o_masks[i] = o;
    o += orbx::scratch_align(H * N);
    o_counts[i] = o;
    o += orbx::scratch_align(sizeof(int) * H);
  }
  const size_t off_back = o;
  for (int i = 0; i < n; i++) {
    o_rec[i] = o;
    o += orbx::scratch_align(sizeof(Sim3Rec) + (size_t)std::max(runs[i].h->N, 1));
  }
  const size_t total = o, back_bytes = total - off_back;
  RANSAC_CHECK(dev.dstage_reserve(total));
  RANSAC_CHECK(dev.pinned_reserve(up_bytes + back_bytes));
  uint8_t* hp = (uint8_t*)dev.pinned;
  uint8_t* dp = (uint8_t*)dev.dstage;
  Sim3Job* jobs = (Sim3Job*)hp;
  for (int i = 0; i < n; i++) {
    orbx_sim3* h = runs[i].h;
    const int N = h->N, H = runs[i].H;
    orbx::ransac_sample_sets(runs[i].rv, H, 3, N, (int*)(hp + o_sets[i]));  // :180-202
    Sim3Job& J = jobs[i];
    J.in = h->in();
    J.sets = (const int*)(dp + o_sets[i]);
    J.hyps = (Sim3Hyp*)(dp + o_hyps[i]);
    J.masks = dp + o_masks[i];
    J.counts = (int*)(dp + o_counts[i]);
    J.state = h->d_state;
    J.best_mask = h->d_best;
    J.rec = (Sim3Rec*)(dp + o_rec[i]);
    J.out_mask = dp + o_rec[i] + sizeof(Sim3Rec);
    J.H = H;
    J.max_its = h->max_its;
    J.min_inliers = h->min_inliers;
    J.too_few = runs[i].too_few;
  }
  RANSAC_CHECK(hipMemcpyAsync(dp, hp, up_bytes, hipMemcpyHostToDevice, st));
  RANSAC_CHECK(hipMemsetAsync(dp + off_back, 0, back_bytes, st));
  if (Hmax > 0)
    hipLaunchKernelGGL(orbx::k_sim3_hyp, dim3(Hmax, n), dim3(orbx::kSim3Threads), 0, st, (const Sim3Job*)dp);
  if (shared)
    hipLaunchKernelGGL(orbx::k_sim3_select, dim3(1), dim3(64 * std::min(n, 16)), 0, st, (const Sim3Job*)dp, n, 1);
  else
    hipLaunchKernelGGL(orbx::k_sim3_select, dim3(n), dim3(64), 0, st, (const Sim3Job*)dp, n, 0);
  RANSAC_CHECK(hipGetLastError());
  uint8_t* back = hp + up_bytes;
  RANSAC_CHECK(hipMemcpyAsync(back, dp + off_back, back_bytes, hipMemcpyDeviceToHost, st));
  RANSAC_CHECK(hipStreamSynchronize(st));
  bool stopped = false;
  for (int i = 0; i < n; i++) {
    Sim3Run& r = runs[i];
    const uint8_t* b = back + (o_rec[i] - off_back);
    if (shared && stopped) {  // never reached by the reference's loop
      std::memset(&r.rec, 0, sizeof(r.rec));
      continue;
    }
    std::memcpy(&r.rec, b, sizeof(Sim3Rec));
    if (!r.too_few) {
      r.h->iterations = r.rec.iterations;
      r.h->best_inliers = r.rec.best_inliers;
    }
    if (r.rec.found) {
      if (inliers && inliers[i]) std::memcpy(inliers[i], b + sizeof(Sim3Rec), (size_t)r.h->N);
      stopped = true;
    }
  }
  return ORBX_OK;
}

orbx_status sim3_check_solvers(orbx_sim3* const* solvers, int n, const void* results) {
  if (n < 0 || (n > 0 && (!solvers || !results))) return ORBX_ERR_ARG;
  for (int i = 0; i < n; i++) {
    if (!solvers[i] || solvers[i]->device != solvers[0]->device) return ORBX_ERR_ARG;
    if (solvers[i]->N >= solvers[i]->min_inliers && solvers[i]->N < 3) return ORBX_ERR_ARG;
    for (int j = 0; j < i; j++)
      if (solvers[j] == solvers[i]) return ORBX_ERR_ARG;
  }
  return ORBX_OK;
}

void sim3_result(const Sim3Run& r, orbx_sim3_result* out) {
  out->no_more = r.rec.no_more;
  out->found = r.rec.found;
  out->n_inliers = r.rec.n_inliers;
  out->used = 3 * r.rec.done;
  std::memcpy(out->T12, r.rec.T12, sizeof(out->T12));
}

}  // namespace

extern "C" {

orbx_status orbx_sim3_create(const orbx_sim3_solver_problem* p, const orbx_sim3_params* prm, int device,
                             orbx_sim3** out) {
  return orbx_sim3_create_many(p, 1, prm, device, out);
}

orbx_status orbx_sim3_create_many(const orbx_sim3_solver_problem* problems, int n, const orbx_sim3_params* prm,
                                  int device, orbx_sim3** out) {
  if (n < 0 || !prm || (n > 0 && (!problems || !out))) return ORBX_ERR_ARG;
  for (int i = 0; i < n; i++) {
    const orbx_status s = sim3_check_problem(&problems[i], prm);
    if (s != ORBX_OK) return s;
  }
  for (int i = 0; i < n; i++) out[i] = nullptr;
  if (n == 0) return ORBX_OK;
  orbx_status s = orbx::ransac_device_check(g_sim3_dev, device, nullptr);
  if (s != ORBX_OK) return s;
  orbx::RansacDevice& dev = g_sim3_dev[device];
  std::lock_guard<std::mutex> lock(dev.mu);
  std::vector<orbx_sim3*> hs(n, nullptr);
  auto fail = [&](orbx_status code) {
    for (orbx_sim3* h : hs) sim3_free(h);
    return code;
  };
  size_t stage = 0;
  for (int i = 0; i < n; i++) {
    hs[i] = sim3_new(&problems[i], prm, device);
    if (!hs[i]) return fail(ORBX_ERR_HIP);
    if (sim3_alloc(hs[i]) != ORBX_OK) return fail(ORBX_ERR_HIP);
    stage += hs[i]->upload_bytes();
  }
  // every solver's correspondences in one pinned block, one upload, one gather launch
  const size_t off_data = orbx::scratch_align(sizeof(Sim3GatherJob) * (size_t)n);
  const size_t bytes = off_data + stage;
  if (dev.pinned_reserve(bytes) != hipSuccess || dev.dstage_reserve(bytes) != hipSuccess) return fail(ORBX_ERR_HIP);
  uint8_t* hp = (uint8_t*)dev.pinned;
  uint8_t* dp = (uint8_t*)dev.dstage;
  Sim3GatherJob* jobs = (Sim3GatherJob*)hp;
  size_t o = off_data;
  for (int i = 0; i < n; i++) {
    const size_t len = hs[i]->upload_bytes();
    std::memset(hp + o, 0, len);
    if (problems[i].n > 0) sim3_stage(hs[i], &problems[i], hp + o);
    jobs[i] = Sim3GatherJob{dp + o, (uint8_t*)hs[i]->d_x1, problems[i].n > 0 ? (int)len : 0};
    o += len;
  }
  hipStream_t st = dev.st;
  if (hipMemcpyAsync(dp, hp, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return fail(ORBX_ERR_HIP);
  hipLaunchKernelGGL(orbx::k_sim3_gather, dim3(n), dim3(256), 0, st, (const Sim3GatherJob*)dp);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(ORBX_ERR_HIP);
  for (int i = 0; i < n; i++) out[i] = hs[i];
  return ORBX_OK;
}

orbx_status orbx_sim3_destroy(orbx_sim3* h) {
  if (!h) return ORBX_ERR_ARG;
  (void)hipSetDevice(h->device);
  sim3_free(h);
  return ORBX_OK;
}

orbx_status orbx_sim3_set_ransac_parameters(orbx_sim3* h, const orbx_sim3_params* prm) {
  if (!h || !prm) return ORBX_ERR_ARG;
  int its;
  if (!sim3_derive(h->N, prm, &its)) return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  std::lock_guard<std::mutex> lock(g_sim3_dev[h->device].mu);
  h->prob = prm->probability;
  h->min_inliers = prm->min_inliers;
  h->max_its = its;
  // :150 mnIterations = 0; the best set, its count and the best Sim3 are kept
  h->iterations = 0;
  RANSAC_CHECK(hipMemsetAsync(&h->d_state->iterations, 0, sizeof(int), h->st));
  return ORBX_OK;
}

orbx_status orbx_sim3_get_params(const orbx_sim3* h, int* min_inliers, int* max_iterations, int* iterations,
                                 int* best_inliers) {
  if (!h) return ORBX_ERR_ARG;
  if (min_inliers) *min_inliers = h->min_inliers;
  if (max_iterations) *max_iterations = h->max_its;
  if (iterations) *iterations = h->iterations;
  if (best_inliers) *best_inliers = h->best_inliers;
  return ORBX_OK;
}

orbx_status orbx_sim3_iterate(orbx_sim3* h, int n_iterations, const int32_t* rand_vals, int n_rand, int* used,
                              int* no_more, float T12[16], uint8_t* inliers, int* n_inliers, int* found) {
  if (!h || !used || !no_more || !T12 || !n_inliers || !found || (h->N > 0 && !inliers) || n_rand < 0 ||
      (n_rand > 0 && !rand_vals))
    return ORBX_ERR_ARG;
  if (h->N >= h->min_inliers && h->N < 3) return ORBX_ERR_ARG;
  *used = *no_more = *n_inliers = *found = 0;
  std::memset(T12, 0, 16 * sizeof(float));
  if (h->N > 0) std::memset(inliers, 0, (size_t)h->N);
  std::vector<Sim3Run> runs(1);
  runs[0].h = h;
  runs[0].rv = rand_vals;
  sim3_begin(runs[0], n_iterations);
  if (runs[0].too_few) {  // :161-165, nothing is drawn and the device is not needed
    *no_more = 1;
    return ORBX_OK;
  }
  if ((long long)runs[0].H * 3 > n_rand) return ORBX_ERR_CAPACITY;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  std::lock_guard<std::mutex> lock(g_sim3_dev[h->device].mu);
  const orbx_status s = sim3_run(runs, false, &inliers);
  if (s != ORBX_OK) return s;
  orbx_sim3_result r;
  sim3_result(runs[0], &r);
  *used = r.used;
  *no_more = r.no_more;
  *n_inliers = r.n_inliers;
  *found = r.found;
  std::memcpy(T12, r.T12, sizeof(r.T12));
  return ORBX_OK;
}

orbx_status orbx_sim3_iterate_stream(orbx_sim3* h, int n_iterations, orbx_rand_state* rng, int* no_more,
                                     float T12[16], uint8_t* inliers, int* n_inliers, int* found) {
  if (!h || !rng) return ORBX_ERR_ARG;
  Sim3Run r;
  r.h = h;
  sim3_begin(r, n_iterations);
  const int need = 3 * r.H;
  const std::vector<int32_t> vals = orbx::rand_peek(rng, need);
  int used = 0;
  const orbx_status st =
      orbx_sim3_iterate(h, n_iterations, vals.data(), need, &used, no_more, T12, inliers, n_inliers, found);
  if (st != ORBX_OK) return st;
  orbx::rand_advance(rng, used);
  return ORBX_OK;
}

orbx_status orbx_sim3_get_estimate(orbx_sim3* h, float R[9], float t[3], float* s) {
  if (!h || !R || !t || !s) return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  std::lock_guard<std::mutex> lock(g_sim3_dev[h->device].mu);
  Sim3Hyp best;
  RANSAC_CHECK(hipMemcpyAsync(&best, &h->d_state->best, sizeof(best), hipMemcpyDeviceToHost, h->st));
  RANSAC_CHECK(hipStreamSynchronize(h->st));
  std::memcpy(R, best.R, sizeof(best.R));
  std::memcpy(t, best.t, sizeof(best.t));
  *s = best.s;
  return ORBX_OK;
}

orbx_status orbx_sim3_iterate_candidates(orbx_sim3* const* solvers, int n, int n_iterations, orbx_rand_state* rng,
                                         orbx_sim3_result* results, uint8_t* const* inliers, int* stopped) {
  orbx_status s = sim3_check_solvers(solvers, n, results);
  if (s != ORBX_OK || !rng || !stopped) return s != ORBX_OK ? s : ORBX_ERR_ARG;
  *stopped = n;
  if (n == 0) return ORBX_OK;
  std::vector<Sim3Run> runs(n);
  size_t total = 0;
  for (int i = 0; i < n; i++) {
    runs[i].h = solvers[i];
    sim3_begin(runs[i], n_iterations);
    total += 3 * (size_t)runs[i].H;
  }
  // solver i draws from where solver i-1 ends when it returns nothing (all of its iterations)
  const std::vector<int32_t> vals = orbx::rand_peek(rng, total);
  size_t o = 0;
  for (int i = 0; i < n; i++) {
    runs[i].rv = vals.data() + o;
    o += 3 * (size_t)runs[i].H;
  }
  if (hipSetDevice(solvers[0]->device) != hipSuccess) return ORBX_ERR_HIP;
  std::lock_guard<std::mutex> lock(g_sim3_dev[solvers[0]->device].mu);
  if ((s = sim3_run(runs, true, inliers)) != ORBX_OK) return s;
  size_t used = 0;
  for (int i = 0; i < n; i++) {
    sim3_result(runs[i], &results[i]);
    if (i <= *stopped) used += (size_t)results[i].used;
    if (results[i].found && *stopped == n) *stopped = i;
  }
  orbx::rand_advance(rng, used);
  return ORBX_OK;
}

orbx_status orbx_sim3_iterate_many(orbx_sim3* const* solvers, int n, int n_iterations, orbx_rand_state* const* rngs,
                                   orbx_sim3_result* results, uint8_t* const* inliers) {
  orbx_status s = sim3_check_solvers(solvers, n, results);
  if (s != ORBX_OK) return s;
  if (n == 0) return ORBX_OK;
  if (!rngs) return ORBX_ERR_ARG;
  for (int i = 0; i < n; i++) {
    if (!rngs[i]) return ORBX_ERR_ARG;
    for (int j = 0; j < i; j++)
      if (rngs[j] == rngs[i]) return ORBX_ERR_ARG;  // independent streams only (shared: _candidates)
  }
  std::vector<Sim3Run> runs(n);
  std::vector<std::vector<int32_t>> vals(n);
  for (int i = 0; i < n; i++) {
    runs[i].h = solvers[i];
    sim3_begin(runs[i], n_iterations);
    vals[i] = orbx::rand_peek(rngs[i], 3 * (size_t)runs[i].H);
    runs[i].rv = vals[i].data();
  }
  if (hipSetDevice(solvers[0]->device) != hipSuccess) return ORBX_ERR_HIP;
  std::lock_guard<std::mutex> lock(g_sim3_dev[solvers[0]->device].mu);
  if ((s = sim3_run(runs, false, inliers)) != ORBX_OK) return s;
  for (int i = 0; i < n; i++) {
    sim3_result(runs[i], &results[i]);
    orbx::rand_advance(rngs[i], results[i].used);
  }
  return ORBX_OK;
}

double orbx_debug_atan2_det(double y, double x) { return orbx::atan2_det(y, x); }

}  // extern "C"

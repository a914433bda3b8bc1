// initializer.hip -- Initializer::Initialize (src/Initializer.cc:58-167) on the GPU: the monocular
// two-view bootstrap that consumes ORBmatcher::SearchForInitialization (src/Tracking.cc:683-730).
//
//   k_init_hyp       one 256-thread block per (iteration, model), 2 * iterations blocks: ComputeH21
//                    (:315-360) or ComputeF21 (:374-421) of the block's 8-point set on lane 0 with the
//                    Jacobi SVD's matrices in LDS, denormalised (and inverted, for H); then
//                    CheckHomography / CheckFundamental (:424-636) of every match by all threads.  The
//                    per-match score terms go to LDS (0 for a skipped add: bit-neutral on a
//                    non-negative running sum) and lane 0 walks them in match order, so the score is
//                    the reference's sequential float sum.
//   k_init_select    one wave: the two first-best walks (`currentScore > score`), RH = SH/(SH+SF) and
//                    the choice, then DecomposeE (:1317-1345, via E = K' F K) or the 8-solution
//                    decomposition of ReconstructH (:792-929): 4 or 8 (R, t) records + the inlier count
//   k_init_check_rt  one block per motion hypothesis (8 launched, the unused ones exit): CheckRT
//                    (:1134-1303), a thread per match with its own 4x4 Jacobi triangulation (LDS
//                    slices), nGood, per-keypoint vP3D / vbGood, the parallax by rank selection
//   k_init_decide    one wave: ReconstructF's / ReconstructH's decision (:685-762, :931-982) and the
//                    winner copied out
// Normalize (:1076-1131) is two strictly sequential float sums over a frame's keypoints; it runs on
// the host (once per frame: at creation for the reference frame, per call for the current one) and
// the normalised points travel with the upload.  One call: one upload (points of frame 2, matches,
// sets), four launches, one readback.
//
// Arithmetic: the OpenCV 3.2 calls restated operation by operation (parity), float and
// double exactly where the library uses them, -ffp-contract=off; acos through acosf_det.  The Jacobi
// SVD is orbx_cvsvd.h's, the template PnP instantiates at double; gemm, inv, det, convertTo, norm and dot
// on 3x3 / 3x1 Mats are orbx_cv.h's.  Every
// routine is __host__ __device__: orbx_debug_initializer_host runs the same code on the host.
// tests/initializer_literal.py is the same sequence in numpy, and both equal it bit for bit.
//
// Bound: latency.  A hypothesis block's life is the serial Jacobi SVD on one lane (16x9: 36 column
// pairs a sweep); the checks read 16 B and write 1 B per match.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/orbx.h"
#include "../../include/orbx_debug.h"
#include "orbx_cv.h"
#include "orbx_cvsvd.h"
#include "orbx_device.h"
#include "orbx_ransac.h"

#define INIT_HD __host__ __device__ __forceinline__

namespace orbx {

struct InitRec {  // select / check_rt / decide results, read back as one record
  int ok, degenerate, model, n_hyp;
  int it_h, it_f, best, n_inliers;
  float SH, SF, pad[2];
  float H21[9], F21[9];
  float R[8][9], t[8][3];
  int n_good[8];
  float parallax[8];
};

struct InitJob {
  const float *k1, *k2;    // mvKeys1 / mvKeys2 (x, y)
  const float *pn1, *pn2;  // Normalize of every keypoint
  const int *m1, *m2;      // mvMatches12: first, second
  const int* sets;         // iterations x 8
  float T1[9], T2inv[9], T2t[9], K[9];
  float sigma, inv_sigma2, th2;
  int N, n1, n2, iterations;
  float* models;   // 2*iterations x 18: H21 | H12, or F21 | unused
  float* scores;   // 2*iterations
  uint8_t* masks;  // 2*iterations x N
  uint32_t* keys;  // 8 x N: init_cos_key of the cosine of a match that passed CheckRT
  float* p3d;      // 8 x n1 x 3
  uint8_t* good;   // 8 x n1
  InitRec* rec;
  float* out_p3d;  // n1 x 3
  uint8_t *out_tri, *out_mh, *out_mf;
};

struct InitRt {  // one motion hypothesis of CheckRT
  float R[9], t[3], P1[12], P2[12], O2[3];
  float fx, fy, cx, cy, th2;
};

// ------------------------------------------------------------------ OpenCV 3.2 pieces
// cv::SVD is orbx_cvsvd.h's JacobiSVDImpl_ at T = float (minval = FLT_MIN, eps = 2 FLT_EPSILON), always
// in its rolled form (kSmall = false): the matrices are run-time indexed memory, LDS on the device.
using cvsvd::jacobi_svd;

// gemm, inv, det, convertTo, norm and dot on 3x3 / 3x1 Mats are orbx_cv.h's (row stride 3 throughout).

// cv::SVD::compute(A, w, u, vt, FULL_UV) of a 3x3 CV_32F.  ws: 18 floats + W: 3 doubles of
// run-time indexed memory (LDS on the device); u, w, vt: the results
INIT_HD void init_svd3(const float* A, float* ws, double* W, float* u, float* w, float* vt) {
  float* B = ws;       // temp_a = A^T
  float* V = ws + 9;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) B[3 * c + r] = A[3 * r + c];
  jacobi_svd<float, 3, 3, 3, true, false>(B, W, V);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      u[3 * r + c] = B[3 * c + r];
      vt[3 * r + c] = V[3 * r + c];
    }
  for (int k = 0; k < 3; k++) w[k] = (float)W[k];
}
constexpr int kInitSvd3Ws = 21;  // 18 + 3 spare (the slices carved after it keep their offsets)

// ------------------------------------------------------------------ hypotheses
constexpr int kInitSolveWs = 9 * 16 + 81 + kInitSvd3Ws + 64;

// ComputeH21 / ComputeF21 of set `it` + the denormalisation of FindHomography (:211-213) /
// FindFundamental (:271-280).  ws, W (9 doubles): run-time indexed memory; M: 18 floats (H21 | H12, F21)
INIT_HD void init_solve(const InitJob& J, int it, int model, float* ws, double* W, float* M) {
  float* At = ws;
  float* Vt = ws + 144;
  float* s3 = ws + 144 + 81;
  float* tmp = s3 + kInitSvd3Ws;  // Fpre / u / w / vt / products (run-time indexed through init_svd3)
  const int* set = J.sets + 8 * (size_t)it;
  if (model == 0) {
    for (int j = 0; j < 8; j++) {
      const int idx = set[j];
      const int a = J.m1[idx], b = J.m2[idx];
      const float u1 = J.pn1[2 * a], v1 = J.pn1[2 * a + 1], u2 = J.pn2[2 * b], v2 = J.pn2[2 * b + 1];
      const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
      const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
#pragma unroll
      for (int c = 0; c < 9; c++) {
        At[16 * c + 2 * j] = r0[c];
        At[16 * c + 2 * j + 1] = r1[c];
      }
    }
    jacobi_svd<float, 16, 9, 0, true, false>(At, W, Vt);
    float Hn[9], P[9], H21[9], H12[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Hn[k] = Vt[72 + k];
    cvmat::gemm33<3>(J.T2inv, Hn, 1.0, P);
    cvmat::gemm33<3>(P, J.T1, 1.0, H21);
    cvmat::inv3<3>(H21, H12);
#pragma unroll
    for (int k = 0; k < 9; k++) M[k] = H21[k], M[9 + k] = H12[k];
  } else {
    for (int j = 0; j < 8; j++) {
      const int idx = set[j];
      const int a = J.m1[idx], b = J.m2[idx];
      const float u1 = J.pn1[2 * a], v1 = J.pn1[2 * a + 1], u2 = J.pn2[2 * b], v2 = J.pn2[2 * b + 1];
      const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
#pragma unroll
      for (int c = 0; c < 9; c++) At[9 * j + c] = r[c];
    }
    for (int c = 0; c < 9; c++) At[72 + c] = 0.f;  // temp_u = Scalar::all(0)
    jacobi_svd<float, 9, 8, 9, false, false>(At, W, nullptr);
    float* Fpre = tmp;
    for (int k = 0; k < 9; k++) Fpre[k] = At[72 + k];
    float u[9], w[3], vt[9];
    init_svd3(Fpre, s3, W, tmp + 9, tmp + 18, tmp + 21);
#pragma unroll
    for (int k = 0; k < 9; k++) u[k] = tmp[9 + k], vt[k] = tmp[21 + k];
    w[0] = tmp[18], w[1] = tmp[19], w[2] = 0.f;
    const float D[9] = {w[0], 0.f, 0.f, 0.f, w[1], 0.f, 0.f, 0.f, w[2]};
    float P[9], Fn[9], F21[9];
    cvmat::gemm33<3>(u, D, 1.0, P);
    cvmat::gemm33<3>(P, vt, 1.0, Fn);
    cvmat::gemm33<3>(J.T2t, Fn, 1.0, P);
    cvmat::gemm33<3>(P, J.T1, 1.0, F21);
#pragma unroll
    for (int k = 0; k < 9; k++) M[k] = F21[k], M[9 + k] = 0.f;
  }
}

// CheckHomography (:466-530) / CheckFundamental (:560-633) of one match: the two score terms
// (0 where the reference skips the add) and bIn
INIT_HD void init_check(int model, const float* M, float u1, float v1, float u2, float v2, float inv_s2, float* t1,
                        float* t2, bool* in) {
  float chi1, chi2, th, th_score;
  if (model == 0) {
    const float* h = M;
    const float* g = M + 9;
    th = th_score = 5.991f;
    const float w2 = (float)(1.0 / (double)(g[6] * u2 + g[7] * v2 + g[8]));
    const float x2 = (g[0] * u2 + g[1] * v2 + g[2]) * w2;
    const float y2 = (g[3] * u2 + g[4] * v2 + g[5]) * w2;
    chi1 = ((u1 - x2) * (u1 - x2) + (v1 - y2) * (v1 - y2)) * inv_s2;
    const float w1 = (float)(1.0 / (double)(h[6] * u1 + h[7] * v1 + h[8]));
    const float x1 = (h[0] * u1 + h[1] * v1 + h[2]) * w1;
    const float y1 = (h[3] * u1 + h[4] * v1 + h[5]) * w1;
    chi2 = ((u2 - x1) * (u2 - x1) + (v2 - y1) * (v2 - y1)) * inv_s2;
  } else {
    const float* f = M;
    th = 3.841f;
    th_score = 5.991f;
    const float a2 = f[0] * u1 + f[1] * v1 + f[2];
    const float b2 = f[3] * u1 + f[4] * v1 + f[5];
    const float c2 = f[6] * u1 + f[7] * v1 + f[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2;
    const float a1 = f[0] * u2 + f[3] * v2 + f[6];
    const float b1 = f[1] * u2 + f[4] * v2 + f[7];
    const float c1 = f[2] * u2 + f[5] * v2 + f[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2;
  }
  const bool o1 = chi1 > th, o2 = chi2 > th;
  *t1 = o1 ? 0.f : th_score - chi1;
  *t2 = o2 ? 0.f : th_score - chi2;
  *in = !(o1 || o2);
}

constexpr int kInitThreads = 256;

__global__ __launch_bounds__(kInitThreads) void k_init_hyp(const InitJob* jp) {
  const InitJob& J = *jp;
  __shared__ float sws[kInitSolveWs];
  __shared__ double sW[9];
  __shared__ float sM[18];
  __shared__ float sTerm[2 * kInitThreads];
  const int h = blockIdx.x, tid = threadIdx.x, N = J.N, its = J.iterations;
  const int model = h >= its, it = model ? h - its : h;
  if (tid == 0) {
    init_solve(J, it, model, sws, sW, sM);
    for (int k = 0; k < 18; k++) J.models[18 * (size_t)h + k] = sM[k];
  }
  __syncthreads();
  uint8_t* mask = J.masks + (size_t)h * N;
  float score = 0.f;
  for (int base = 0; base < N; base += kInitThreads) {
    const int i = base + tid;
    if (i < N) {
      const int a = J.m1[i], b = J.m2[i];
      float t1, t2;
      bool in;
      init_check(model, sM, J.k1[2 * a], J.k1[2 * a + 1], J.k2[2 * b], J.k2[2 * b + 1], J.inv_sigma2, &t1, &t2, &in);
      sTerm[2 * tid] = t1;
      sTerm[2 * tid + 1] = t2;
      mask[i] = in;
    }
    __syncthreads();
    if (tid == 0) {
      const int cnt = 2 * min(kInitThreads, N - base);
      for (int k = 0; k < cnt; k++) score += sTerm[k];
    }
    __syncthreads();
  }
  if (tid == 0) J.scores[h] = score;
}

// ------------------------------------------------------------------ select
// The part of Initialize after the two Find* (:156-164) and the head of ReconstructF (:659-669) /
// ReconstructH (:792-929): the motion hypotheses.  ws: kInitSvd3Ws + 27 floats, W: 3 doubles.
INIT_HD void init_motion(const InitJob& J, InitRec* rec, float* ws, double* W, int it_h, float SH, int it_f, float SF) {
  rec->it_h = it_h;
  rec->it_f = it_f;
  rec->SH = SH;
  rec->SF = SF;
  rec->ok = 0;
  rec->best = -1;
  rec->n_hyp = 0;
  rec->n_inliers = 0;
  rec->degenerate = 0;
  rec->model = -1;
  const int its = J.iterations;
  for (int k = 0; k < 9; k++) {
    rec->H21[k] = it_h >= 0 ? J.models[18 * (size_t)it_h + k] : 0.f;
    rec->F21[k] = it_f >= 0 ? J.models[18 * (size_t)(its + it_f) + k] : 0.f;
  }
  if (it_h < 0 && it_f < 0) {
    rec->degenerate = 1;
    return;
  }
  const float RH = SH / (SH + SF);
  float* s3 = ws;
  float* uu = ws + kInitSvd3Ws;  // u | w | vt | (3 spare)
  float K[9], u[9], w[3], vt[9];
#pragma unroll
  for (int k = 0; k < 9; k++) K[k] = J.K[k];
  if (!((double)RH > 0.40)) {
    rec->model = 1;
    float F[9], P[9], E[9];
#pragma unroll
    for (int k = 0; k < 9; k++) F[k] = rec->F21[k];
    // K.t()*F21: GEMMSingleMul<float,double> (GEMM_1_T), then the small path by K
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += (double)K[3 * k + i] * (double)F[3 * k + j];
        P[3 * i + j] = (float)(s * 1.0);
      }
    cvmat::gemm33<3>(P, K, 1.0, E);
    // DecomposeE
    for (int k = 0; k < 9; k++) ws[kInitSvd3Ws + 30 + k] = E[k];
    init_svd3(ws + kInitSvd3Ws + 30, s3, W, uu, uu + 9, uu + 12);
#pragma unroll
    for (int k = 0; k < 9; k++) u[k] = uu[k], vt[k] = uu[12 + k];
    float t[3] = {u[2], u[5], u[8]};
    const double nt = cvmat::norm3(t);
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = cvmat::scale(t[k], 1.0 / nt);
    const float Wm[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float R1[9], R2[9];
    cvmat::gemm33<3>(u, Wm, 1.0, P);
    cvmat::gemm33<3>(P, vt, 1.0, R1);
    if (cvmat::det3<3>(R1) < 0)
#pragma unroll
      for (int k = 0; k < 9; k++) R1[k] = cvmat::scale(R1[k], -1.0);
    cvmat::gemm33_bt<3>(u, Wm, 1.0, P);  // u*W.t(): GEMM_2_T
    cvmat::gemm33<3>(P, vt, 1.0, R2);
    if (cvmat::det3<3>(R2) < 0)
#pragma unroll
      for (int k = 0; k < 9; k++) R2[k] = cvmat::scale(R2[k], -1.0);
    float t2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) t2[k] = cvmat::scale(t[k], -1.0);
#pragma unroll
    for (int k = 0; k < 9; k++) {
      rec->R[0][k] = R1[k];
      rec->R[1][k] = R2[k];
      rec->R[2][k] = R1[k];
      rec->R[3][k] = R2[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      rec->t[0][k] = t[k];
      rec->t[1][k] = t[k];
      rec->t[2][k] = t2[k];
      rec->t[3][k] = t2[k];
    }
    rec->n_hyp = 4;
    return;
  }
  rec->model = 0;
  float H[9], invK[9], P[9], A[9];
#pragma unroll
  for (int k = 0; k < 9; k++) H[k] = rec->H21[k];
  cvmat::inv3<3>(K, invK);
  cvmat::gemm33<3>(invK, H, 1.0, P);
  cvmat::gemm33<3>(P, K, 1.0, A);
  for (int k = 0; k < 9; k++) ws[kInitSvd3Ws + 30 + k] = A[k];
  init_svd3(ws + kInitSvd3Ws + 30, s3, W, uu, uu + 9, uu + 12);
#pragma unroll
  for (int k = 0; k < 9; k++) u[k] = uu[k], vt[k] = uu[12 + k];
#pragma unroll
  for (int k = 0; k < 3; k++) w[k] = uu[9 + k];
  const float s = (float)(cvmat::det3<3>(u) * cvmat::det3<3>(vt));
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return;
  const float aux1 = __builtin_sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const float aux3 = __builtin_sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const float x1[4] = {aux1, aux1, -aux1, -aux1};
  const float x3[4] = {aux3, -aux3, aux3, -aux3};
  const float aux_st = __builtin_sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
  const float ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const float st[4] = {aux_st, -aux_st, -aux_st, aux_st};
  const float aux_sp = __builtin_sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
  const float cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
  const float sp[4] = {aux_sp, -aux_sp, -aux_sp, aux_sp};
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int j = i & 3;
    float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    float tp[3];
    if (i < 4) {
      Rp[0] = ct, Rp[2] = -st[j], Rp[6] = st[j], Rp[8] = ct;
      const double f = (double)(d1 - d3);
      tp[0] = cvmat::scale(x1[j], f), tp[1] = cvmat::scale(0.f, f), tp[2] = cvmat::scale(-x3[j], f);
    } else {
      Rp[0] = cp, Rp[2] = sp[j], Rp[4] = -1.f, Rp[6] = sp[j], Rp[8] = -cp;
      const double f = (double)(d1 + d3);
      tp[0] = cvmat::scale(x1[j], f), tp[1] = cvmat::scale(0.f, f), tp[2] = cvmat::scale(x3[j], f);
    }
    float R[9], t[3];
    cvmat::gemm33<3>(u, Rp, (double)s, P);
    cvmat::gemm33<3>(P, vt, 1.0, R);
    cvmat::gemm31<3>(u, tp, 1.0, t);
    const double nt = cvmat::norm3(t);
#pragma unroll
    for (int k = 0; k < 9; k++) rec->R[i][k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) rec->t[i][k] = cvmat::scale(t[k], 1.0 / nt);
  }
  rec->n_hyp = 8;
}
constexpr int kInitMotionWs = kInitSvd3Ws + 30 + 9;

__global__ __launch_bounds__(64) void k_init_select(const InitJob* jp) {
  const InitJob& J = *jp;
  __shared__ float sws[kInitMotionWs];
  __shared__ double sW[3];
  __shared__ int s_pick[3];
  const int lane = threadIdx.x, its = J.iterations, N = J.N;
  int bi[2];
  float bs[2];
  // the first-best walks (:219, :287): the first hypothesis that reaches the largest score above 0
  for (int model = 0; model < 2; model++) {
    bi[model] = -1;
    bs[model] = 0.f;
    for (int base = 0; base < its; base += 64) {
      const int k = base + lane;
      float s = k < its ? J.scores[(size_t)model * its + k] : -1.f;
      if (!(s > 0.f)) s = -1.f;
      int idx = k;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float s2 = __shfl_xor(s, o, 64);
        const int i2 = __shfl_xor(idx, o, 64);
        if (s2 > s || (s2 == s && i2 < idx)) s = s2, idx = i2;
      }
      if (s > bs[model]) bs[model] = s, bi[model] = idx;
    }
  }
  InitRec* rec = J.rec;
  if (lane == 0) {
    init_motion(J, rec, sws, sW, bi[0], bs[0], bi[1], bs[1]);
    s_pick[0] = rec->model;
  }
  __syncthreads();
  const int model = s_pick[0];
  const uint8_t* mh = bi[0] >= 0 ? J.masks + (size_t)bi[0] * N : nullptr;
  const uint8_t* mf = bi[1] >= 0 ? J.masks + (size_t)(its + bi[1]) * N : nullptr;
  int cnt = 0;
  for (int i = lane; i < N; i += 64) {
    const uint8_t a = mh ? mh[i] : 0, b = mf ? mf[i] : 0;
    J.out_mh[i] = a;
    J.out_mf[i] = b;
    cnt += model == 0 ? a : (model == 1 ? b : 0);
  }
  cnt = wave_sum(cnt);
  if (lane == 0) rec->n_inliers = cnt;
}

// ------------------------------------------------------------------ CheckRT
// P1 = K[I|0], P2 = K*[R|t] (GEMMSingleMul<float,double>: 3x4 leaves the small path), O2 = -R.t()*t
INIT_HD void init_rt_setup(const float* K, float th2, const float* R, const float* t, InitRt* C) {
  for (int k = 0; k < 9; k++) C->R[k] = R[k];
  for (int k = 0; k < 3; k++) C->t[k] = t[k];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      C->P1[4 * i + j] = j < 3 ? K[3 * i + j] : 0.f;
      double s = 0;
      for (int k = 0; k < 3; k++) s += (double)K[3 * i + k] * (double)(j < 3 ? R[3 * k + j] : t[k]);
      C->P2[4 * i + j] = (float)(s * 1.0);
    }
  cvmat::gemm31_at<3, true>(R, t, -1.0, C->O2);
  C->fx = K[0], C->fy = K[4], C->cx = K[2], C->cy = K[5];
  C->th2 = th2;
}

// One match of CheckRT's loop (:1186-1282) with Triangulate (:1018-1064).  At, Vt (16 floats each,
// row stride 4) and W (4 doubles): run-time indexed memory.  Returns bit 0: counted in nGood (X
// is vP3D's entry), bit 1: cosParallax < 0.99998 (vbGood).
INIT_HD int init_rt_point(const InitRt& C, float x1, float y1, float x2, float y2, float* At, float* Vt, double* W,
                          float X[3], float* cosp) {
  // x*P.row(2) - P.row(r): addWeighted, (a*x + b*(-1.0f)) + 0.0f; a - b when x == 1
  for (int c = 0; c < 4; c++) {
    const float p12 = C.P1[8 + c], p22 = C.P2[8 + c];
    At[4 * c + 0] = x1 == 1.f ? p12 - C.P1[c] : (p12 * x1 + C.P1[c] * -1.0f) + 0.0f;
    At[4 * c + 1] = y1 == 1.f ? p12 - C.P1[4 + c] : (p12 * y1 + C.P1[4 + c] * -1.0f) + 0.0f;
    At[4 * c + 2] = x2 == 1.f ? p22 - C.P2[c] : (p22 * x2 + C.P2[c] * -1.0f) + 0.0f;
    At[4 * c + 3] = y2 == 1.f ? p22 - C.P2[4 + c] : (p22 * y2 + C.P2[4 + c] * -1.0f) + 0.0f;
  }
  jacobi_svd<float, 4, 4, 0, true, false>(At, W, Vt);
  const double iw = 1.0 / (double)Vt[15];
  X[0] = cvmat::scale(Vt[12], iw);
  X[1] = cvmat::scale(Vt[13], iw);
  X[2] = cvmat::scale(Vt[14], iw);
  *cosp = 0.f;
  if (!__builtin_isfinite(X[0]) || !__builtin_isfinite(X[1]) || !__builtin_isfinite(X[2])) return 0;
  const float n1[3] = {X[0] - 0.f, X[1] - 0.f, X[2] - 0.f};
  const float dist1 = (float)cvmat::norm3(n1);
  const float n2[3] = {X[0] - C.O2[0], X[1] - C.O2[1], X[2] - C.O2[2]};
  const float dist2 = (float)cvmat::norm3(n2);
  const float cosParallax = (float)(cvmat::dot<3>(n1, n2) / (double)(dist1 * dist2));
  *cosp = cosParallax;
  const bool low = (double)cosParallax < 0.99998;
  if (X[2] <= 0 && low) return 0;
  float X2[3];
  cvmat::gemm31_add<3>(C.R, X, 1.0, C.t, X2);
  if (X2[2] <= 0 && low) return 0;
  const float invZ1 = (float)(1.0 / (double)X[2]);
  const float im1x = C.fx * X[0] * invZ1 + C.cx, im1y = C.fy * X[1] * invZ1 + C.cy;
  const float e1 = (im1x - x1) * (im1x - x1) + (im1y - y1) * (im1y - y1);
  if (e1 > C.th2) return 0;
  const float invZ2 = (float)(1.0 / (double)X2[2]);
  const float im2x = C.fx * X2[0] * invZ2 + C.cx, im2y = C.fy * X2[1] * invZ2 + C.cy;
  const float e2 = (im2x - x2) * (im2x - x2) + (im2y - y2) * (im2y - y2);
  if (e2 > C.th2) return 0;
  return 1 | (low ? 2 : 0);
}

// The order of the sorted cosines (:1289) as unsigned keys: numbers ascending (-0 counts as +0), NaN
// after every number (std::sort on NaN is undefined; the literal's numpy.sort does the same), and
// 0xFFFFFFFF for a match that did not pass.  Element k of the sorted list is the value x with
// #(keys < x) <= k < #(keys <= x), whichever of equal elements a sort would have put there.
constexpr uint32_t kInitKeyNone = 0xFFFFFFFFu, kInitKeyNaN = 0xFFFFFFFEu;
INIT_HD uint32_t init_cos_key(float c) {
  if (c != c) return kInitKeyNaN;
  c = c + 0.0f;
  uint32_t b;
  __builtin_memcpy(&b, &c, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
INIT_HD float init_key_cos(uint32_t k) {
  uint32_t b = k == kInitKeyNaN ? 0x7FC00000u : ((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
  float c;
  __builtin_memcpy(&c, &b, 4);
  return c;
}

// parallax = acos(vCosParallax[idx])*180/CV_PI (:1296)
INIT_HD float init_parallax(float c) { return (float)((double)(acosf_det(c) * 180.f) / 3.1415926535897932384626433832795); }

__global__ __launch_bounds__(kInitThreads) void k_init_check_rt(const InitJob* jp) {
  const InitJob& J = *jp;
  InitRec* rec = J.rec;
  const int b = blockIdx.x;
  if (b >= rec->n_hyp) return;  // block-uniform
  __shared__ float sA[kInitThreads * 33];
  __shared__ double sWd[kInitThreads * 5];
  __shared__ InitRt C;
  __shared__ int red[kInitThreads / 64];
  __shared__ uint32_t s_sel;
  const int tid = threadIdx.x, N = J.N, n1 = J.n1;
  const int model = rec->model;
  const uint8_t* mask = J.masks + ((size_t)model * J.iterations + (model ? rec->it_f : rec->it_h)) * N;
  float* p3d = J.p3d + (size_t)b * n1 * 3;
  uint8_t* good = J.good + (size_t)b * n1;
  uint32_t* keys = J.keys + (size_t)b * N;
  if (tid == 0) {
    init_rt_setup(J.K, J.th2, rec->R[b], rec->t[b], &C);
    s_sel = kInitKeyNone;
  }
  for (int i = tid; i < 3 * n1; i += kInitThreads) p3d[i] = 0.f;
  for (int i = tid; i < n1; i += kInitThreads) good[i] = 0;
  __syncthreads();
  int cnt = 0;
  for (int i = tid; i < N; i += kInitThreads) {
    uint32_t key = kInitKeyNone;
    float cp = 0.f;
    if (mask[i]) {
      const int a = J.m1[i], c = J.m2[i];
      float X[3];
      const int st = init_rt_point(C, J.k1[2 * a], J.k1[2 * a + 1], J.k2[2 * c], J.k2[2 * c + 1], sA + 33 * tid,
                                   sA + 33 * tid + 16, sWd + 5 * tid, X, &cp);
      if (st & 1) {
        cnt++;
        key = init_cos_key(cp);
        p3d[3 * a] = X[0], p3d[3 * a + 1] = X[1], p3d[3 * a + 2] = X[2];
        if (st & 2) good[a] = 1;
      }
    }
    keys[i] = key;
  }
  cnt = wave_sum(cnt);
  if ((tid & 63) == 0) red[tid >> 6] = cnt;
  __threadfence_block();
  __syncthreads();
  const int nGood = red[0] + red[1] + red[2] + red[3];
  if (nGood > 0) {  // block-uniform
    // element min(50, size - 1) of the sorted cosines (:1289-1296) by rank; the keys are staged in
    // the triangulation's LDS when they fit (every thread walks all of them: broadcast reads)
    const uint32_t* kk = keys;
    if (N <= kInitThreads * 33) {
      uint32_t* sk = (uint32_t*)sA;
      for (int i = tid; i < N; i += kInitThreads) sk[i] = keys[i];
      __syncthreads();
      kk = sk;
    }
    const int target = min(50, nGood - 1);
    for (int i = tid; i < N; i += kInitThreads) {
      const uint32_t ki = kk[i];
      if (ki == kInitKeyNone) continue;
      int less = 0, leq = 0;
      for (int j = 0; j < N; j++) {
        const uint32_t kj = kk[j];
        less += kj < ki;
        leq += kj <= ki;
      }
      if (less <= target && target < leq) s_sel = ki;  // equal keys: the same bits from every writer
    }
  }
  __syncthreads();
  if (tid == 0) {
    rec->n_good[b] = nGood;
    rec->parallax[b] = nGood > 0 ? init_parallax(init_key_cos(s_sel)) : 0.f;
  }
}

// ------------------------------------------------------------------ decide
// The tails of ReconstructF (:685-762) and ReconstructH (:931-982): the hypothesis copied out, or -1
INIT_HD int init_decide(const InitRec& rec) {
  const float minParallax = 1.0f;
  const int minTriangulated = 50, N = rec.n_inliers;
  if (rec.n_hyp == 4) {
    const int* g = rec.n_good;
    const int maxGood = max(g[0], max(g[1], max(g[2], g[3])));
    const int nMinGood = max((int)(0.9 * N), minTriangulated);
    int nsimilar = 0;
    for (int k = 0; k < 4; k++)
      if (g[k] > 0.7 * maxGood) nsimilar++;
    if (maxGood < nMinGood || nsimilar > 1) return -1;
    for (int k = 0; k < 4; k++)
      if (maxGood == g[k]) return rec.parallax[k] > minParallax ? k : -1;
    return -1;
  }
  if (rec.n_hyp == 8) {
    int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
    float bestParallax = -1;
    for (int i = 0; i < 8; i++) {
      const int nGood = rec.n_good[i];
      if (nGood > bestGood) {
        secondBestGood = bestGood;
        bestGood = nGood;
        bestSolutionIdx = i;
        bestParallax = rec.parallax[i];
      } else if (nGood > secondBestGood) {
        secondBestGood = nGood;
      }
    }
    if (secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > minTriangulated &&
        bestGood > 0.9 * N)
      return bestSolutionIdx;
  }
  return -1;
}

__global__ __launch_bounds__(64) void k_init_decide(const InitJob* jp) {
  const InitJob& J = *jp;
  InitRec* rec = J.rec;
  __shared__ int s_best;
  const int lane = threadIdx.x, n1 = J.n1;
  if (lane == 0) {
    const int best = init_decide(*rec);
    rec->best = best;
    rec->ok = best >= 0;
    s_best = best;
  }
  __syncthreads();
  const int best = s_best;
  if (best < 0) return;
  const float* p = J.p3d + (size_t)best * n1 * 3;
  const uint8_t* g = J.good + (size_t)best * n1;
  for (int i = lane; i < 3 * n1; i += 64) J.out_p3d[i] = p[i];
  for (int i = lane; i < n1; i += 64) J.out_tri[i] = g[i];
}

}  // namespace orbx

// ------------------------------------------------------------------ host / C ABI
namespace {

using orbx::InitJob;
using orbx::InitRec;

orbx::RansacDevice* const g_init_dev = new orbx::RansacDevice[64];  // never deleted (orbx_mem.h)

// Normalize (:1076-1131) over every keypoint of a frame: float accumulators in index order
void init_normalize(const float* keys, int n, float* pn, float T[9]) {
  float meanX = 0, meanY = 0;
  for (int i = 0; i < n; i++) {
    meanX += keys[2 * i];
    meanY += keys[2 * i + 1];
  }
  meanX = meanX / n;
  meanY = meanY / n;
  float meanDevX = 0, meanDevY = 0;
  for (int i = 0; i < n; i++) {
    pn[2 * i] = keys[2 * i] - meanX;
    pn[2 * i + 1] = keys[2 * i + 1] - meanY;
    meanDevX += std::fabs(pn[2 * i]);
    meanDevY += std::fabs(pn[2 * i + 1]);
  }
  meanDevX = meanDevX / n;
  meanDevY = meanDevY / n;
  const float sX = (float)(1.0 / meanDevX), sY = (float)(1.0 / meanDevY);
  for (int i = 0; i < n; i++) {
    pn[2 * i] = pn[2 * i] * sX;
    pn[2 * i + 1] = pn[2 * i + 1] * sY;
  }
  const float t[9] = {sX, 0.f, -meanX * sX, 0.f, sY, -meanY * sY, 0.f, 0.f, 1.f};
  std::memcpy(T, t, sizeof(t));
}

}  // namespace

struct orbx_initializer {
  int device = -1;  // -1: the host twin
  int n1 = 0, iterations = 0;
  float K[9], sigma = 1.f, T1[9];
  std::vector<float> k1, pn1;
  orbx::DevBuf<float> d_mem;  // k1 | pn1
};

namespace {

orbx_status init_check_create(const float* keys1_xy, int n1, const float* K, int iterations) {
  if (!keys1_xy || !K || n1 < 8 || iterations < 1 || iterations > (1 << 20) || n1 > (1 << 24)) return ORBX_ERR_ARG;
  return ORBX_OK;
}

void init_fill(orbx_initializer* h, const float* keys1_xy, int n1, const float* K, float sigma, int iterations) {
  h->n1 = n1;
  h->iterations = iterations;
  h->sigma = sigma;
  std::memcpy(h->K, K, sizeof(h->K));
  h->k1.assign(keys1_xy, keys1_xy + 2 * (size_t)n1);
  h->pn1.resize(2 * (size_t)n1);
  init_normalize(keys1_xy, n1, h->pn1.data(), h->T1);
}

// What one Initialize call stages on the host: the match list (:73-84), the sets (:109-131), the
// current frame's Normalize, T2.inv() and T2.t().
struct InitCall {
  int N = 0;
  std::vector<int> m1, m2, sets;
  std::vector<float> pn2;
  InitJob J;
};

orbx_status init_prepare(const orbx_initializer* h, const float* keys2_xy, int n2, const int32_t* matches12,
                         const int32_t* rand_vals, int n_rand, InitCall& c) {
  if (!h || !keys2_xy || !matches12 || n2 < 1 || n2 > (1 << 24) || n_rand < 0 || (n_rand > 0 && !rand_vals))
    return ORBX_ERR_ARG;
  for (int i = 0; i < h->n1; i++)
    if (matches12[i] >= 0) {
      if (matches12[i] >= n2) return ORBX_ERR_ARG;
      c.m1.push_back(i);
      c.m2.push_back(matches12[i]);
    }
  c.N = (int)c.m1.size();
  if (c.N < 8) return ORBX_ERR_ARG;
  const int need = 8 * h->iterations;
  if (n_rand < need) return ORBX_ERR_CAPACITY;
  for (int k = 0; k < need; k++)
    if (rand_vals[k] < 0) return ORBX_ERR_ARG;
  c.sets.resize((size_t)need);
  orbx::ransac_sample_sets(rand_vals, h->iterations, 8, c.N, c.sets.data());
  c.pn2.resize(2 * (size_t)n2);
  float T2[9];
  init_normalize(keys2_xy, n2, c.pn2.data(), T2);
  InitJob& J = c.J;
  std::memset(&J, 0, sizeof(J));
  std::memcpy(J.T1, h->T1, sizeof(J.T1));
  orbx::cvmat::inv3<3>(T2, J.T2inv);
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) J.T2t[3 * r + k] = T2[3 * k + r];
  std::memcpy(J.K, h->K, sizeof(J.K));
  J.sigma = h->sigma;
  J.inv_sigma2 = (float)(1.0 / (h->sigma * h->sigma));
  const float sigma2 = h->sigma * h->sigma;
  J.th2 = (float)(4.0 * sigma2);
  J.N = c.N;
  J.n1 = h->n1;
  J.n2 = n2;
  J.iterations = h->iterations;
  return ORBX_OK;
}

void init_result(const InitRec& rec, int N, orbx_initializer_result* out, const uint8_t* mh, const uint8_t* mf,
                 float* R21, float* t21) {
  out->ok = rec.ok;
  out->degenerate = rec.degenerate;
  out->SH = rec.SH;
  out->SF = rec.SF;
  std::memcpy(out->H21, rec.H21, sizeof(out->H21));
  std::memcpy(out->F21, rec.F21, sizeof(out->F21));
  out->it_h = rec.it_h;
  out->it_f = rec.it_f;
  out->model = rec.model;
  out->n_hyp = rec.n_hyp;
  for (int k = 0; k < 8; k++) {
    out->n_good[k] = k < rec.n_hyp ? rec.n_good[k] : 0;
    out->parallax[k] = k < rec.n_hyp ? rec.parallax[k] : 0.f;
  }
  out->best = rec.best;
  out->n_matches = N;
  out->n_inliers = rec.n_inliers;
  if (out->inliers_h) std::memcpy(out->inliers_h, mh, (size_t)N);
  if (out->inliers_f) std::memcpy(out->inliers_f, mf, (size_t)N);
  if (rec.ok) {
    std::memcpy(R21, rec.R[rec.best], 9 * sizeof(float));
    std::memcpy(t21, rec.t[rec.best], 3 * sizeof(float));
  }
}

// the device call: one upload, four launches, one readback
orbx_status init_run_device(orbx_initializer* h, const float* keys2_xy, InitCall& c, float* R21, float* t21,
                            float* p3d, uint8_t* tri, orbx_initializer_result* result) {
  orbx::RansacDevice& dev = g_init_dev[h->device];
  hipStream_t st = dev.st;
  const size_t N = c.N, n1 = h->n1, n2 = c.J.n2, its = h->iterations;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += orbx::scratch_align(bytes);
    return at;
  };
  const size_t o_job = take(sizeof(InitJob)), o_k2 = take(8 * n2), o_pn2 = take(8 * n2), o_m1 = take(4 * N),
               o_m2 = take(4 * N), o_sets = take(32 * its);
  const size_t up_bytes = o;
  const size_t o_models = take(72 * 2 * its), o_scores = take(8 * its), o_masks = take(2 * its * N),
               o_keys = take(32 * N), o_p3d = take(96 * n1), o_good = take(8 * n1);
  const size_t off_back = o;
  const size_t o_rec = take(sizeof(InitRec)), o_op3d = take(12 * n1), o_otri = take(n1), o_omh = take(N),
               o_omf = take(N);
  const size_t total = o, back_bytes = total - off_back;
  RANSAC_CHECK(dev.dstage_reserve(total));
  RANSAC_CHECK(dev.pinned_reserve(up_bytes + back_bytes));
  uint8_t* hp = (uint8_t*)dev.pinned;
  uint8_t* dp = (uint8_t*)dev.dstage;
  std::memcpy(hp + o_k2, keys2_xy, 8 * n2);
  std::memcpy(hp + o_pn2, c.pn2.data(), 8 * n2);
  std::memcpy(hp + o_m1, c.m1.data(), 4 * N);
  std::memcpy(hp + o_m2, c.m2.data(), 4 * N);
  std::memcpy(hp + o_sets, c.sets.data(), 32 * its);
  InitJob& J = c.J;
  J.k1 = h->d_mem.p;
  J.pn1 = h->d_mem.p + 2 * n1;
  J.k2 = (const float*)(dp + o_k2);
  J.pn2 = (const float*)(dp + o_pn2);
  J.m1 = (const int*)(dp + o_m1);
  J.m2 = (const int*)(dp + o_m2);
  J.sets = (const int*)(dp + o_sets);
  J.models = (float*)(dp + o_models);
  J.scores = (float*)(dp + o_scores);
  J.masks = dp + o_masks;
  J.keys = (uint32_t*)(dp + o_keys);
  J.p3d = (float*)(dp + o_p3d);
  J.good = dp + o_good;
  J.rec = (InitRec*)(dp + o_rec);
  J.out_p3d = (float*)(dp + o_op3d);
  J.out_tri = dp + o_otri;
  J.out_mh = dp + o_omh;
  J.out_mf = dp + o_omf;
  std::memcpy(hp + o_job, &J, sizeof(J));
  RANSAC_CHECK(hipMemcpyAsync(dp, hp, up_bytes, hipMemcpyHostToDevice, st));
  RANSAC_CHECK(hipMemsetAsync(dp + off_back, 0, back_bytes, st));
  const InitJob* dj = (const InitJob*)(dp + o_job);
  hipLaunchKernelGGL(orbx::k_init_hyp, dim3(2 * (unsigned)its), dim3(orbx::kInitThreads), 0, st, dj);
  hipLaunchKernelGGL(orbx::k_init_select, dim3(1), dim3(64), 0, st, dj);
  hipLaunchKernelGGL(orbx::k_init_check_rt, dim3(8), dim3(orbx::kInitThreads), 0, st, dj);
  hipLaunchKernelGGL(orbx::k_init_decide, dim3(1), dim3(64), 0, st, dj);
  RANSAC_CHECK(hipGetLastError());
  uint8_t* back = hp + up_bytes;
  RANSAC_CHECK(hipMemcpyAsync(back, dp + off_back, back_bytes, hipMemcpyDeviceToHost, st));
  RANSAC_CHECK(hipStreamSynchronize(st));
  InitRec rec;
  std::memcpy(&rec, back + (o_rec - off_back), sizeof(rec));
  init_result(rec, c.N, result, back + (o_omh - off_back), back + (o_omf - off_back), R21, t21);
  if (rec.ok) {
    std::memcpy(p3d, back + (o_op3d - off_back), 12 * n1);
    std::memcpy(tri, back + (o_otri - off_back), n1);
  }
  return ORBX_OK;
}

// the same stages on the host, in the kernels' order
void init_run_host(const orbx_initializer* h, const float* keys2_xy, InitCall& c, float* R21, float* t21, float* p3d,
                   uint8_t* tri, orbx_initializer_result* result) {
  const int N = c.N, n1 = h->n1, its = h->iterations;
  InitJob& J = c.J;
  std::vector<float> models(36 * (size_t)its), scores(2 * (size_t)its), P(3 * (size_t)n1 * 8);
  std::vector<uint32_t> keys(N);
  std::vector<uint8_t> masks(2 * (size_t)its * N), good((size_t)n1 * 8), zero(N, 0);
  InitRec rec;
  std::memset(&rec, 0, sizeof(rec));
  J.k1 = h->k1.data();
  J.pn1 = h->pn1.data();
  J.k2 = keys2_xy;
  J.pn2 = c.pn2.data();
  J.m1 = c.m1.data();
  J.m2 = c.m2.data();
  J.sets = c.sets.data();
  J.models = models.data();
  J.scores = scores.data();
  J.masks = masks.data();
  J.rec = &rec;
  float ws[orbx::kInitSolveWs];
  double W[16];
  for (int hh = 0; hh < 2 * its; hh++) {
    const int model = hh >= its, it = model ? hh - its : hh;
    float* M = models.data() + 18 * (size_t)hh;
    orbx::init_solve(J, it, model, ws, W, M);
    float score = 0.f;
    for (int i = 0; i < N; i++) {
      const int a = c.m1[i], b = c.m2[i];
      float t1, t2;
      bool in;
      orbx::init_check(model, M, J.k1[2 * a], J.k1[2 * a + 1], J.k2[2 * b], J.k2[2 * b + 1], J.inv_sigma2, &t1, &t2,
                       &in);
      score += t1;
      score += t2;
      masks[(size_t)hh * N + i] = in;
    }
    scores[hh] = score;
  }
  int bi[2] = {-1, -1};
  float bs[2] = {0.f, 0.f};
  for (int model = 0; model < 2; model++)
    for (int k = 0; k < its; k++)
      if (scores[(size_t)model * its + k] > bs[model]) bs[model] = scores[(size_t)model * its + k], bi[model] = k;
  float mws[orbx::kInitMotionWs];
  orbx::init_motion(J, &rec, mws, W, bi[0], bs[0], bi[1], bs[1]);
  const uint8_t* mh = bi[0] >= 0 ? masks.data() + (size_t)bi[0] * N : zero.data();
  const uint8_t* mf = bi[1] >= 0 ? masks.data() + (size_t)(its + bi[1]) * N : zero.data();
  const uint8_t* mask = rec.model == 0 ? mh : mf;
  for (int i = 0; i < N && rec.model >= 0; i++) rec.n_inliers += mask[i];
  for (int b = 0; b < rec.n_hyp; b++) {
    orbx::InitRt C;
    orbx::init_rt_setup(J.K, J.th2, rec.R[b], rec.t[b], &C);
    float* pb = P.data() + (size_t)b * n1 * 3;
    uint8_t* gb = good.data() + (size_t)b * n1;
    int nGood = 0;
    for (int i = 0; i < N; i++) {
      keys[i] = orbx::kInitKeyNone;
      if (!mask[i]) continue;
      const int a = c.m1[i], cc = c.m2[i];
      float X[3], At[16], Vt[16], cp;
      const int st = orbx::init_rt_point(C, J.k1[2 * a], J.k1[2 * a + 1], J.k2[2 * cc], J.k2[2 * cc + 1], At, Vt, W, X,
                                         &cp);
      if (st & 1) {
        nGood++;
        keys[i] = orbx::init_cos_key(cp);
        pb[3 * a] = X[0], pb[3 * a + 1] = X[1], pb[3 * a + 2] = X[2];
        if (st & 2) gb[a] = 1;
      }
    }
    uint32_t sel = orbx::kInitKeyNone;
    if (nGood > 0) {
      const int target = std::min(50, nGood - 1);
      for (int i = 0; i < N; i++) {
        if (keys[i] == orbx::kInitKeyNone) continue;
        int less = 0, leq = 0;
        for (int j = 0; j < N; j++) less += keys[j] < keys[i], leq += keys[j] <= keys[i];
        if (less <= target && target < leq) sel = keys[i];
      }
    }
    rec.n_good[b] = nGood;
    rec.parallax[b] = nGood > 0 ? orbx::init_parallax(orbx::init_key_cos(sel)) : 0.f;
  }
  rec.best = orbx::init_decide(rec);
  rec.ok = rec.best >= 0;
  init_result(rec, N, result, mh, mf, R21, t21);
  if (rec.ok) {
    std::memcpy(p3d, P.data() + (size_t)rec.best * n1 * 3, 12 * (size_t)n1);
    std::memcpy(tri, good.data() + (size_t)rec.best * n1, (size_t)n1);
  }
}

}  // namespace

extern "C" {

orbx_status orbx_initializer_create(const float* keys1_xy, int n1, const float K[9], float sigma, int iterations,
                                    int device, orbx_initializer** out) {
  if (!out) return ORBX_ERR_ARG;
  *out = nullptr;
  orbx_status s = init_check_create(keys1_xy, n1, K, iterations);
  if (s != ORBX_OK) return s;
  if ((s = orbx::ransac_device_check(g_init_dev, device, nullptr)) != ORBX_OK) return s;
  orbx::RansacDevice& dev = g_init_dev[device];
  std::lock_guard<std::mutex> lock(dev.mu);
  orbx_initializer* h = new (std::nothrow) orbx_initializer();
  if (!h) return ORBX_ERR_HIP;
  init_fill(h, keys1_xy, n1, K, sigma, iterations);
  h->device = device;
  const size_t half = 8 * (size_t)n1;
  if (h->d_mem.ensure(4 * (size_t)n1) != hipSuccess ||
      hipMemcpyAsync(h->d_mem.p, h->k1.data(), half, hipMemcpyHostToDevice, dev.st) != hipSuccess ||
      hipMemcpyAsync(h->d_mem.p + 2 * (size_t)n1, h->pn1.data(), half, hipMemcpyHostToDevice, dev.st) != hipSuccess ||
      hipStreamSynchronize(dev.st) != hipSuccess) {
    delete h;
    return ORBX_ERR_HIP;
  }
  *out = h;
  return ORBX_OK;
}

orbx_status orbx_initializer_destroy(orbx_initializer* h) {
  if (!h) return ORBX_ERR_ARG;
  if (h->device >= 0) (void)hipSetDevice(h->device);
  delete h;
  return ORBX_OK;
}

orbx_status orbx_initializer_initialize(orbx_initializer* h, const float* keys2_xy, int n2, const int32_t* matches12,
                                        const int32_t* rand_vals, int n_rand, int* used, float R21[9], float t21[3],
                                        float* p3d, uint8_t* triangulated, orbx_initializer_result* result) {
  if (!h || h->device < 0 || !used || !R21 || !t21 || !p3d || !triangulated || !result) return ORBX_ERR_ARG;
  *used = 0;
  InitCall c;
  const orbx_status s = init_prepare(h, keys2_xy, n2, matches12, rand_vals, n_rand, c);
  if (s != ORBX_OK) return s;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  std::lock_guard<std::mutex> lock(g_init_dev[h->device].mu);
  const orbx_status r = init_run_device(h, keys2_xy, c, R21, t21, p3d, triangulated, result);
  if (r == ORBX_OK) *used = 8 * h->iterations;
  return r;
}

orbx_status orbx_initializer_initialize_stream(orbx_initializer* h, const float* keys2_xy, int n2,
                                               const int32_t* matches12, orbx_rand_state* rng, float R21[9],
                                               float t21[3], float* p3d, uint8_t* triangulated,
                                               orbx_initializer_result* result) {
  if (!h || !rng) return ORBX_ERR_ARG;
  const int need = 8 * h->iterations;
  const std::vector<int32_t> vals = orbx::rand_peek(rng, (size_t)need);
  int used = 0;
  const orbx_status s =
      orbx_initializer_initialize(h, keys2_xy, n2, matches12, vals.data(), need, &used, R21, t21, p3d, triangulated,
                                  result);
  if (s != ORBX_OK) return s;
  orbx::rand_advance(rng, (size_t)used);
  return ORBX_OK;
}

int orbx_debug_initializer_host(const float* keys1_xy, int n1, const float K[9], float sigma, int iterations,
                                const float* keys2_xy, int n2, const int32_t* matches12, const int32_t* rand_vals,
                                int n_rand, int* used, float R21[9], float t21[3], float* p3d,
                                uint8_t* triangulated, orbx_initializer_result* result) {
  if (!used || !R21 || !t21 || !p3d || !triangulated || !result) return ORBX_ERR_ARG;
  *used = 0;
  orbx_status s = init_check_create(keys1_xy, n1, K, iterations);
  if (s != ORBX_OK) return s;
  orbx_initializer h;
  init_fill(&h, keys1_xy, n1, K, sigma, iterations);
  InitCall c;
  if ((s = init_prepare(&h, keys2_xy, n2, matches12, rand_vals, n_rand, c)) != ORBX_OK) return s;
  init_run_host(&h, keys2_xy, c, R21, t21, p3d, triangulated, result);
  *used = 8 * iterations;
  return ORBX_OK;
}

float orbx_debug_acosf_det(float x) { return orbx::acosf_det(x); }

}  // extern "C"

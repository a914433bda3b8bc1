// newpoints.hip -- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:281-558), the consumer of
// ORBmatcher::SearchForTriangulation, as one chain of launches on one stream:
//
//   k_cnmp_gate                 one 256-thread block per neighbour, all neighbours in one launch (nothing
//                               here depends on the chain): KeyFrame::SetPose's Rwc / Ow of both
//                               keyframes (src/KeyFrame.cc:80-101), vBaseline and its norm, the stereo
//                               gate (:339) or the monocular one (:346-352) with
//                               ComputeSceneMedianDepth(2) (src/KeyFrame.cc:784-819: the depths by all
//                               threads, the element of rank (n-1)/2 by rank counting, which no thread
//                               order can change), ComputeF12 (:672-699); the neighbour's
//                               orbx_tri_problem is completed on the device.  A skipped neighbour's
//                               problem is emptied, so its search block leaves at once.
//   k_search_for_triangulation  triangulation.hip's kernel, unchanged, one launch per neighbour, reading
//                               the chain's has_mp1.
//   k_cnmp_points               one 256-thread block per neighbour: the matched pairs compacted in
//                               ascending idx1, then :383-556 per pair (a thread per pair, its 4x4 Jacobi
//                               SVD in an LDS slice), the accepted ones written in the reference's order
//                               by a ballot scan (no claimed slots), has_mp1[idx1] set for the later
//                               neighbours, and MapPoint::UpdateNormalAndDepth of the two observations
//                               (src/MapPoint.cc:343-393).  Its last act is the CheckNewKeyFrames() of
//                               the NEXT neighbour (:320): the search is reused unchanged, so the flag is
//                               read at the tail of the launch before it, not at its head; a raised flag
//                               sets a device word and empties the remaining search problems.
// k_cnmp_points is one workgroup per neighbour on purpose: a neighbour has a few hundred pairs at most (one
// or two rounds of a thread per pair), the chain is bound by its launches, and one block makes the ordered
// compaction a ballot scan with no second launch and no block waiting for another.  (A thread per feature
// of KF1 over several workgroups would need a cross-block scan.)
// No block waits for another: the stream alone orders the launches.  One call: one upload, 1 + 2 n
// launches, one readback.
//
// Arithmetic: OpenCV 3.2's calls restated operation by operation as tests/newpoints_literal.py lists
// them (the small Mat arithmetic is orbx_cv.h's, the ordered compaction orbx_device.h's compact_chunk),
// -ffp-contract=off.  cos / atan2 at :410-412 are the float overloads (DBoW2's
// TemplatedVocabulary.h puts `using namespace std` in front of the translation unit, so
// atan2(float, float) and cos(float) resolve to std's float forms): (float)atan2_det in double, the
// doubling in float, (float) of sincos_d's cosine.  Every routine is __host__ __device__:
// orbx_debug_new_points_host runs the same text on the host.
//
// Bound: latency -- a chain of short launches, each a few hundred independent pairs at most.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "../../include/orbx.h"
#include "../../include/orbx_debug.h"
#include "orbx_cv.h"
#include "orbx_cvsvd.h"
#include "orbx_device.h"
#include "orbx_scratch.h"

#define CN_HD __host__ __device__ __forceinline__

namespace orbx {
namespace tri {
// triangulation.hip: k_search_for_triangulation over n device-resident problems, one block each
hipError_t launch_search(const orbx_tri_problem* device_problems, int n, hipStream_t st);
}  // namespace tri

namespace cnmp {

using cvsvd::jacobi_svd;
using namespace cvmat;  // OpenCV 3.2's gemm, inv, convertTo, norm and dot (orbx_cv.h), row stride 3 throughout
typedef orbx_new_points_kf Kf;

struct Pose {  // KeyFrame::SetPose
  float Rcw[9], tcw[3], Rwc[9], Ow[3], invfx, invfy;
};

struct PairOut {
  float X[3], cosr, cos1, cos2, normal[3], dmin, dmax;
};

struct Job {
  Kf cur;
  const Kf* nb;  // n_nb
  int n_nb, monocular, raise_after, zstride;
  float ratio_factor;
  const int* flag;        // two host-mapped words (the handle's flag, the mirror of a caller's bool); may be null
  orbx_tri_problem* tri;  // n_nb
  Pose* pose;             // 1 + n_nb
  float* zbuf;            // n_nb x zstride
  int32_t* match12;       // n_nb x n1
  int32_t* nmatches;      // n_nb
  int32_t* pairs;         // n1
  int32_t* ctl;           // [0]: stopped
  int32_t *n_new, *nb_done, *pt_idx;
  float *pt_pos, *pt_normal, *pt_dist;
  int32_t *nb_skip, *nb_nm;
  float *nb_base, *nb_med;
  uint8_t* has_mp1;
  uint8_t* pr_exit;  // probes (null: off)
  float *pr_cos, *pr_f12;
};

// ------------------------------------------------------------------ the gate
// KeyFrame::SetPose: Rwc = Rcw.t() (a Mat of its own), Ow = -Rwc*tcw = gemm(Rwc, tcw, alpha = -1)
CN_HD void cn_pose(const Kf& K, Pose* P) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      P->Rcw[3 * r + c] = K.Tcw[4 * r + c];
      P->Rwc[3 * c + r] = K.Tcw[4 * r + c];
    }
    P->tcw[r] = K.Tcw[4 * r + 3];
  }
  gemm31<3>(P->Rwc, P->tcw, -1.0, P->Ow);
  P->invfx = 1.0f / K.fx;
  P->invfy = 1.0f / K.fy;
}
// ComputeSceneMedianDepth's z = Rcw2.dot(x3Dw) + zcw
CN_HD float cn_depth(const Pose& P, const float* x) { return (float)(dot<3>(P.Rcw + 6, x) + (double)P.tcw[2]); }
CN_HD float cn_baseline(const Pose& P1, const Pose& P2) {
  const float v[3] = {P2.Ow[0] - P1.Ow[0], P2.Ow[1] - P1.Ow[1], P2.Ow[2] - P1.Ow[2]};
  return (float)norm3(v);
}
CN_HD int cn_gate_code(int monocular, float baseline, float mb2, int n_depths, float median) {
  if (!monocular) return baseline < mb2 ? ORBX_NP_NB_BASELINE : ORBX_NP_NB_RAN;
  if (n_depths <= 0) return ORBX_NP_NB_NO_DEPTHS;
  const float ratioBaselineDepth = baseline / median;
  return (double)ratioBaselineDepth < 0.01 ? ORBX_NP_NB_RATIO : ORBX_NP_NB_RAN;
}
// ComputeF12: R12 = R1w*R2w.t(); t12 = gemm(gemm(R1w, R2w.t(), alpha = -1), t2w, 1, t1w, 1) as the MatExpr
// folds -R1w*R2w.t()*t2w+t1w; K1.t().inv()*t12x*R12*K2.inv() left to right
CN_HD void cn_f12(const Kf& K1, const Pose& P1, const Kf& K2, const Pose& P2, float* F) {
  float R12[9], M[9], t12[3];
  gemm33_bt<3>(P1.Rcw, P2.Rcw, 1.0, R12);
  gemm33_bt<3>(P1.Rcw, P2.Rcw, -1.0, M);
  gemm31_add<3>(M, P2.tcw, 1.0, P1.tcw, t12);
  const float tx[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};
  const float K1t[9] = {K1.fx, 0.f, 0.f, 0.f, K1.fy, 0.f, K1.cx, K1.cy, 1.f};
  const float K2m[9] = {K2.fx, 0.f, K2.cx, 0.f, K2.fy, K2.cy, 0.f, 0.f, 1.f};
  float A[9], B[9], C[9], K2i[9];
  inv3<3>(K1t, A);
  gemm33<3>(A, tx, 1.0, B);
  gemm33<3>(B, R12, 1.0, C);
  inv3<3>(K2m, K2i);
  gemm33<3>(C, K2i, 1.0, F);
}
// what SearchForTriangulation reads beside the two keyframes
CN_HD void cn_fill_tri(const Kf& K2, const Pose& P1, const float* F, int ran, orbx_tri_problem* T) {
  for (int k = 0; k < 9; k++) T->F12[k] = F[k];
  for (int k = 0; k < 3; k++) T->C1w[k] = P1.Ow[k];
  for (int k = 0; k < 16; k++) T->T2w[k] = K2.Tcw[k];
  T->fx = K2.fx, T->fy = K2.fy, T->cx = K2.cx, T->cy = K2.cy;
  for (int k = 0; k < 16; k++) {
    T->scale_factors2[k] = K2.scale_factors[k];
    T->level_sigma2_2[k] = K2.level_sigma2[k];
  }
  if (!ran) T->kf1.n = T->kf1.n_nodes = T->kf2.n_nodes = 0;
}

// ------------------------------------------------------------------ one matched pair (:383-556)
// cos(2*atan2(mb/2, depth)) in the float overloads
CN_HD float cn_cos_stereo(float mb, float depth) {
  const float a = (float)atan2_det((double)(mb / 2), (double)depth);
  const float t = 2 * a;
  double s, c;
  sincos_d((double)t, &s, &c);
  return (float)c;
}
// KeyFrame::UnprojectStereo on the distorted mvKeys: gemm(Rwc, x3Dc, 1, Ow, 1)
CN_HD void cn_unproject(const Kf& K, const Pose& P, int i, float z, float* X) {
  const float u = K.keys_xy ? K.keys_xy[2 * i] : K.kf.keys_un[i].x;
  const float v = K.keys_xy ? K.keys_xy[2 * i + 1] : K.kf.keys_un[i].y;
  const float xc[3] = {(u - K.cx) * z * P.invfx, (v - K.cy) * z * P.invfy, z};
  gemm31_add<3>(P.Rwc, xc, 1.0, P.Ow, X);
}
// x*P.row(2) - P.row(r): addWeighted, (a*x + b*(-1.0f)) + 0.0f; a - b when x == 1
CN_HD float cn_row(float x, float p2, float pr) { return x == 1.f ? p2 - pr : (p2 * x + pr * -1.0f) + 0.0f; }

// At, Vt (16 floats each, row stride 4) and W (4 doubles): run-time indexed memory (LDS on the device).
// Returns the pair's ORBX_NP_* code; o->cos* are always written, the rest for an accepted pair.
CN_HD int cn_pair(const Kf& K1, const Pose& P1, const Kf& K2, const Pose& P2, float ratioFactor, int idx1, int idx2,
                  float* At, float* Vt, double* W, PairOut* o) {
  orbx_keypoint kp1 = K1.kf.keys_un[idx1], kp2 = K2.kf.keys_un[idx2];
  kp1.octave &= 15;  // (the level tables hold 16 entries; the host forms have checked the octaves)
  kp2.octave &= 15;
  const float kp1_ur = K1.kf.u_right ? K1.kf.u_right[idx1] : -1.f;
  const float kp2_ur = K2.kf.u_right ? K2.kf.u_right[idx2] : -1.f;
  const bool bStereo1 = kp1_ur >= 0, bStereo2 = kp2_ur >= 0;
  const float xn1[3] = {(kp1.x - K1.cx) * P1.invfx, (kp1.y - K1.cy) * P1.invfy, 1.0f};
  const float xn2[3] = {(kp2.x - K2.cx) * P2.invfx, (kp2.y - K2.cy) * P2.invfy, 1.0f};
  float ray1[3], ray2[3];
  gemm31<3>(P1.Rwc, xn1, 1.0, ray1);
  gemm31<3>(P2.Rwc, xn2, 1.0, ray2);
  const float cosParallaxRays = (float)(dot<3>(ray1, ray2) / (norm3(ray1) * norm3(ray2)));
  float cosParallaxStereo = cosParallaxRays + 1;
  float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
  const float depth1 = K1.depth ? K1.depth[idx1] : -1.f, depth2 = K2.depth ? K2.depth[idx2] : -1.f;
  if (bStereo1)
    cosParallaxStereo1 = cn_cos_stereo(K1.mb, depth1);
  else if (bStereo2)
    cosParallaxStereo2 = cn_cos_stereo(K2.mb, depth2);
  cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;  // std::min
  o->cosr = cosParallaxRays, o->cos1 = cosParallaxStereo1, o->cos2 = cosParallaxStereo2;

  float X[3];
  int how;
  if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 &&
      (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
    for (int c = 0; c < 4; c++) {  // A^T: JacobiSVDImpl_ works on the transpose
      At[4 * c + 0] = cn_row(xn1[0], K1.Tcw[8 + c], K1.Tcw[c]);
      At[4 * c + 1] = cn_row(xn1[1], K1.Tcw[8 + c], K1.Tcw[4 + c]);
      At[4 * c + 2] = cn_row(xn2[0], K2.Tcw[8 + c], K2.Tcw[c]);
      At[4 * c + 3] = cn_row(xn2[1], K2.Tcw[8 + c], K2.Tcw[4 + c]);
    }
    jacobi_svd<float, 4, 4, 0, true, false>(At, W, Vt);
    if (Vt[15] == 0) return ORBX_NP_W_ZERO;
    const double iw = 1.0 / (double)Vt[15];
    X[0] = scale(Vt[12], iw);
    X[1] = scale(Vt[13], iw);
    X[2] = scale(Vt[14], iw);
    how = ORBX_NP_TRIANGULATED;
  } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
    if (!(depth1 > 0)) return ORBX_NP_DEPTH_GUARD;
    cn_unproject(K1, P1, idx1, depth1, X);
    how = ORBX_NP_UNPROJECT1;
  } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
    if (!(depth2 > 0)) return ORBX_NP_DEPTH_GUARD;
    cn_unproject(K2, P2, idx2, depth2, X);
    how = ORBX_NP_UNPROJECT2;
  } else {
    return ORBX_NP_LOW_PARALLAX;
  }

  const float z1 = (float)(dot<3>(P1.Rcw + 6, X) + (double)P1.tcw[2]);
  if (z1 <= 0) return ORBX_NP_Z1;
  const float z2 = (float)(dot<3>(P2.Rcw + 6, X) + (double)P2.tcw[2]);
  if (z2 <= 0) return ORBX_NP_Z2;

  const float sigmaSquare1 = K1.level_sigma2[kp1.octave];
  const float x1 = (float)(dot<3>(P1.Rcw, X) + (double)P1.tcw[0]);
  const float y1 = (float)(dot<3>(P1.Rcw + 3, X) + (double)P1.tcw[1]);
  const float invz1 = (float)(1.0 / (double)z1);
  if (!bStereo1) {
    const float u1 = K1.fx * x1 * invz1 + K1.cx, v1 = K1.fy * y1 * invz1 + K1.cy;
    const float errX1 = u1 - kp1.x, errY1 = v1 - kp1.y;
    if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigmaSquare1) return ORBX_NP_REPROJ1_MONO;
  } else {
    const float u1 = K1.fx * x1 * invz1 + K1.cx;
    const float u1_r = u1 - K1.mbf * invz1;
    const float v1 = K1.fy * y1 * invz1 + K1.cy;
    const float errX1 = u1 - kp1.x, errY1 = v1 - kp1.y, errX1_r = u1_r - kp1_ur;
    if ((double)(errX1 * errX1 + errY1 * errY1 + errX1_r * errX1_r) > 7.8 * (double)sigmaSquare1)
      return ORBX_NP_REPROJ1_STEREO;
  }
  const float sigmaSquare2 = K2.level_sigma2[kp2.octave];
  const float x2 = (float)(dot<3>(P2.Rcw, X) + (double)P2.tcw[0]);
  const float y2 = (float)(dot<3>(P2.Rcw + 3, X) + (double)P2.tcw[1]);
  const float invz2 = (float)(1.0 / (double)z2);
  if (!bStereo2) {
    const float u2 = K2.fx * x2 * invz2 + K2.cx, v2 = K2.fy * y2 * invz2 + K2.cy;
    const float errX2 = u2 - kp2.x, errY2 = v2 - kp2.y;
    if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)sigmaSquare2) return ORBX_NP_REPROJ2_MONO;
  } else {
    const float u2 = K2.fx * x2 * invz2 + K2.cx;
    const float u2_r = u2 - K1.mbf * invz2;  // mpCurrentKeyFrame->mbf, as the reference has it (:509)
    const float v2 = K2.fy * y2 * invz2 + K2.cy;
    const float errX2 = u2 - kp2.x, errY2 = v2 - kp2.y, errX2_r = u2_r - kp2_ur;
    if ((double)(errX2 * errX2 + errY2 * errY2 + errX2_r * errX2_r) > 7.8 * (double)sigmaSquare2)
      return ORBX_NP_REPROJ2_STEREO;
  }

  const float normal1[3] = {X[0] - P1.Ow[0], X[1] - P1.Ow[1], X[2] - P1.Ow[2]};
  const double n1d = norm3(normal1);
  const float dist1 = (float)n1d;
  const float normal2[3] = {X[0] - P2.Ow[0], X[1] - P2.Ow[1], X[2] - P2.Ow[2]};
  const double n2d = norm3(normal2);
  const float dist2 = (float)n2d;
  if (dist1 == 0 || dist2 == 0) return ORBX_NP_DIST_ZERO;
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = K1.scale_factors[kp1.octave] / K2.scale_factors[kp2.octave];
  if (ratioDist * ratioFactor < ratioOctave) return ORBX_NP_RATIO_BELOW;
  if (ratioDist > ratioOctave * ratioFactor) return ORBX_NP_RATIO_ABOVE;

  // MapPoint::UpdateNormalAndDepth of the observations (KF1, idx1), (KF2, idx2): normal = normal +
  // normali/norm is addWeighted(normal, 1, normali, 1/norm), (a*1.0f + b*(float)beta) + 0.0f -- the sum
  // of two terms from zero is the same in either map order; mNormalVector = normal/2 is convertTo(0.5)
  const float b1 = (float)(1.0 / n1d), b2 = (float)(1.0 / n2d);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float s1 = (0.f * 1.0f + normal1[k] * b1) + 0.0f;
    const float s2 = (s1 * 1.0f + normal2[k] * b2) + 0.0f;
    o->normal[k] = scale(s2, 1.0 / 2);
    o->X[k] = X[k];
  }
  o->dmax = dist1 * K1.scale_factors[kp1.octave];
  o->dmin = o->dmax / K1.scale_factors[K1.n_levels - 1];
  return how;
}

// ------------------------------------------------------------------ kernels
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void k_cnmp_gate(const Job* jp) {
  const Job& J = *jp;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b == 0 && tid == 0) {
    *J.n_new = 0;
    *J.nb_done = 0;
    J.ctl[0] = 0;
  }
  if (b >= J.n_nb) return;  // (a launch for no neighbour: the zeroing above)
  __shared__ Pose s_p1, s_p2;
  __shared__ int s_n;
  __shared__ float s_med;
  const Kf& K2 = J.nb[b];
  if (tid == 0) {
    cn_pose(J.cur, &s_p1);
    cn_pose(K2, &s_p2);
    s_n = 0;
    s_med = 0.f;
  }
  __syncthreads();
  if (J.monocular && K2.kf.has_mp && K2.mp_pos) {
    float* z = J.zbuf + (size_t)b * J.zstride;
    const int n2 = K2.kf.n;
    int cnt = 0;
    for (int i = tid; i < n2; i += kThreads)
      if (K2.kf.has_mp[i]) {
        z[i] = cn_depth(s_p2, K2.mp_pos + 3 * (size_t)i);
        cnt++;
      }
    if (cnt) atomicAdd(&s_n, cnt);
    __syncthreads();
    const int n = s_n, k = (n - 1) / 2;
    // sorted[k] is the value v with #(< v) <= k < #(<= v): equal values all write the same bits
    for (int i = tid; i < n2 && n > 0; i += kThreads)
      if (K2.kf.has_mp[i]) {
        const float v = z[i];
        int lt = 0, le = 0;
        for (int j = 0; j < n2; j++)
          if (K2.kf.has_mp[j]) {
            const float w = z[j];
            lt += w < v;
            le += w <= v;
          }
        if (lt <= k && k < le) s_med = v;
      }
    __syncthreads();
  }
  if (tid == 0) {
    const float baseline = cn_baseline(s_p1, s_p2);
    const int code = cn_gate_code(J.monocular, baseline, K2.mb, s_n, s_med);
    float F[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (code == ORBX_NP_NB_RAN) cn_f12(J.cur, s_p1, K2, s_p2, F);
    cn_fill_tri(K2, s_p1, F, code == ORBX_NP_NB_RAN, &J.tri[b]);
    J.nb_skip[b] = code;
    J.nb_base[b] = baseline;
    J.nb_med[b] = J.monocular && code != ORBX_NP_NB_NO_DEPTHS ? s_med : 0.f;
    J.pose[1 + b] = s_p2;
    if (b == 0) J.pose[0] = s_p1;
    if (J.pr_f12)
      for (int k = 0; k < 9; k++) J.pr_f12[9 * b + k] = F[k];
  }
}

__global__ __launch_bounds__(kThreads) void k_cnmp_points(const Job* jp, int nbi) {
  const Job& J = *jp;
  __shared__ float sA[kThreads * 33];
  __shared__ double sW[kThreads * 5];
  __shared__ int s_w[kThreads / 64];
  const int tid = threadIdx.x, n1 = J.cur.kf.n;
  int32_t* m12 = J.match12 + (size_t)nbi * n1;
  const bool stopped = J.ctl[0] != 0;
  const int skip = stopped ? ORBX_NP_NB_STOPPED : J.nb_skip[nbi];
  if (skip != ORBX_NP_NB_RAN) {
    for (int i = tid; i < n1; i += kThreads) m12[i] = -1;
    if (tid == 0) {
      J.nb_nm[nbi] = 0;
      if (stopped) {
        J.nb_skip[nbi] = ORBX_NP_NB_STOPPED;
        J.nb_base[nbi] = 0.f;
        J.nb_med[nbi] = 0.f;
        if (J.pr_f12)
          for (int k = 0; k < 9; k++) J.pr_f12[9 * nbi + k] = 0.f;
      }
    }
  } else {
    const Kf& K2 = J.nb[nbi];
    const Pose P1 = J.pose[0], P2 = J.pose[1 + nbi];
    // the matched pairs in ascending idx1 (vMatchedIndices)
    int np = 0;
    for (int base = 0; base < n1; base += kThreads) {
      const int i = base + tid;
      const bool f = i < n1 && m12[i] >= 0 && m12[i] < K2.kf.n;
      compact_chunk<kThreads>(f, s_w, np, [&](int slot) { J.pairs[slot] = i; });
    }  // (the chunk's closing barrier: the block's J.pairs stores before its loads)
    int n_new = *J.n_new;
    for (int kb = 0; kb < np; kb += kThreads) {
      const int k = kb + tid;
      int code = ORBX_NP_NONE, idx1 = 0, idx2 = 0;
      PairOut o;
      if (k < np) {
        idx1 = J.pairs[k];
        idx2 = m12[idx1];
        float* At = sA + tid * 33;
        code = cn_pair(J.cur, P1, K2, P2, J.ratio_factor, idx1, idx2, At, At + 16, sW + tid * 5, &o);
        if (J.pr_exit) {
          const size_t q = (size_t)nbi * n1 + idx1;
          J.pr_exit[q] = (uint8_t)code;
          J.pr_cos[3 * q] = o.cosr;
          J.pr_cos[3 * q + 1] = o.cos1;
          J.pr_cos[3 * q + 2] = o.cos2;
        }
      }
      const bool acc = code >= ORBX_NP_TRIANGULATED && code <= ORBX_NP_UNPROJECT2;
      int end = n_new, slot = n1;  // end: n_new + the chunk's accepted pairs
      compact_chunk<kThreads>(acc, s_w, end, [&](int s) { slot = s; });
      if (slot < n1) {  // (a feature gets one point at most: the bound always holds); the point's stores
                        // follow the chunk's closing barrier, which need not wait for them
        const size_t s = (size_t)slot;
        J.pt_idx[3 * s] = nbi;
        J.pt_idx[3 * s + 1] = idx1;
        J.pt_idx[3 * s + 2] = idx2;
        for (int c = 0; c < 3; c++) {
          J.pt_pos[3 * s + c] = o.X[c];
          J.pt_normal[3 * s + c] = o.normal[c];
        }
        J.pt_dist[2 * s] = o.dmin;
        J.pt_dist[2 * s + 1] = o.dmax;
        J.has_mp1[idx1] = 1;
      }
      n_new = end < n1 ? end : n1;  // (saturates with the guard above: n_new never counts a point that was
                                    // not written)
    }
    if (tid == 0) {
      *J.n_new = n_new;
      J.nb_nm[nbi] = np;
    }
  }
  if (tid == 0 && !stopped) {
    *J.nb_done = nbi + 1;
    if (nbi + 1 < J.n_nb) {  // CheckNewKeyFrames() of the next neighbour
      bool raised = J.raise_after >= 0 && nbi >= J.raise_after;
      if (J.flag)
        raised |= __hip_atomic_load(J.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0 ||
                  __hip_atomic_load(J.flag + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
      if (raised) {
        J.ctl[0] = 1;
        for (int j = nbi + 1; j < J.n_nb; j++) J.tri[j].kf1.n = J.tri[j].kf1.n_nodes = J.tri[j].kf2.n_nodes = 0;
      }
    }
  }
}

}  // namespace cnmp
}  // namespace orbx

// ------------------------------------------------------------------ C ABI
struct orbx_new_points {
  int device = 0;
  orbx::PinnedBuf flags{true};  // mapped, two ints: [0] the handle's flag, [1] the mirror of a caller's bool
  orbx_new_points_debug_options opt{-1, 0};
  // probes of the last host call
  bool have_probes = false;
  std::vector<uint8_t> pr_exit;
  std::vector<float> pr_cos, pr_f12;
  std::vector<int32_t> pr_m12;
};

namespace {

using orbx::Staging;
using orbx::cnmp::Job;
using orbx::cnmp::Kf;
using orbx::cnmp::Pose;

orbx_status np_check_sizes(const orbx_new_points_problem* p) {
  if (!p) return ORBX_ERR_ARG;
  if (p->n_neighbours < 0) return ORBX_ERR_ARG;
  if (p->n_neighbours > ORBX_NEW_POINTS_MAX_NEIGHBOURS) return ORBX_ERR_SIZE;
  if (p->n_neighbours > 0 && !p->neighbours) return ORBX_ERR_ARG;
  for (int s = 0; s <= p->n_neighbours; s++) {
    const Kf& k = s ? p->neighbours[s - 1] : p->current;
    if (k.kf.n < 0 || k.kf.n_nodes < 0) return ORBX_ERR_ARG;
    if (k.kf.n > ORBX_NEW_POINTS_MAX_FEATURES || k.kf.n_nodes > ORBX_NEW_POINTS_MAX_FEATURES) return ORBX_ERR_SIZE;
    if (k.n_levels < 1 || k.n_levels > 16) return ORBX_ERR_ARG;
  }
  return ORBX_OK;
}

// host arrays: what the kernels trust
orbx_status np_check_host(const orbx_new_points_problem* p) {
  for (int s = 0; s <= p->n_neighbours; s++) {
    const Kf& K = s ? p->neighbours[s - 1] : p->current;
    const orbx_tri_kf& k = K.kf;
    if (k.n > 0 && (!k.keys_un || !k.desc)) return ORBX_ERR_ARG;
    if (k.n_nodes > 0 && (!k.node_id || !k.node_off || !k.feat)) return ORBX_ERR_ARG;
    if (k.u_right && !K.depth) return ORBX_ERR_ARG;
    if (s && p->monocular && k.has_mp && !K.mp_pos) return ORBX_ERR_ARG;
    if (k.n_nodes > 0 && (k.node_off[0] != 0 || k.node_off[k.n_nodes] < 0)) return ORBX_ERR_ARG;
    for (int j = 0; j < k.n_nodes; j++)
      if (k.node_off[j + 1] < k.node_off[j]) return ORBX_ERR_ARG;
    const int nf = k.n_nodes ? k.node_off[k.n_nodes] : 0;
    for (int j = 0; j < nf; j++)
      if (k.feat[j] < 0 || k.feat[j] >= k.n) return ORBX_ERR_ARG;
    for (int i = 0; i < k.n; i++)
      if (k.keys_un[i].octave < 0 || k.keys_un[i].octave >= K.n_levels) return ORBX_ERR_ARG;
  }
  return ORBX_OK;
}

bool np_result_ok(const orbx_new_points_problem* p, const orbx_new_points_result* r) {
  if (!r || !r->n_new || !r->neighbours_done) return false;
  if (p->current.kf.n > 0 && (!r->point_idx || !r->point_pos || !r->point_normal || !r->point_dist || !r->has_mp1))
    return false;
  if (p->n_neighbours > 0 && (!r->nb_skip || !r->nb_nmatches || !r->nb_baseline || !r->nb_median_depth)) return false;
  return true;
}

// the 1 + 2 n launches; `job` is the device copy of J
hipError_t np_enqueue(const Job& J, const Job* job, hipStream_t st) {
  using namespace orbx;
  hipLaunchKernelGGL(cnmp::k_cnmp_gate, dim3(J.n_nb > 0 ? J.n_nb : 1), dim3(cnmp::kThreads), 0, st, job);
  hipError_t e = hipGetLastError();
  for (int i = 0; i < J.n_nb && e == hipSuccess; i++) {
    e = tri::launch_search(J.tri + i, 1, st);
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(cnmp::k_cnmp_points, dim3(1), dim3(cnmp::kThreads), 0, st, job, i);
    e = hipGetLastError();
  }
  return e;
}

void np_tri_pointers(const Job& J, int i, orbx_tri_problem* T) {
  std::memset(T, 0, sizeof(*T));
  T->kf1 = J.cur.kf;
  T->kf1.has_mp = J.has_mp1;
  T->only_stereo = 0;
  T->check_ori = 0;  // ORBmatcher matcher(0.6, false)
  T->match12 = J.match12 + (size_t)i * J.cur.kf.n;
  T->nmatches = J.nmatches + i;
}

orbx_status np_run_host(orbx_new_points* h, const orbx_new_points_problem* p, const orbx_new_points_result* r,
                        const volatile bool* stop) {
  if (!h) return ORBX_ERR_ARG;
  orbx_status cs = np_check_sizes(p);
  if (cs != ORBX_OK) return cs;
  if (!np_result_ok(p, r)) return ORBX_ERR_ARG;
  cs = np_check_host(p);
  if (cs != ORBX_OK) return cs;
  cs = orbx::select_device(h->device);
  if (cs != ORBX_OK) return cs;
  const int nn = p->n_neighbours;
  const size_t n1 = (size_t)p->current.kf.n;
  const bool probes = h->opt.probes != 0;
  Staging S(h->device);
  struct Side {
    Staging::Slot<orbx_keypoint> keys;
    Staging::Slot<uint8_t> desc, has_mp;
    Staging::Slot<float> ur, xy, depth, mp;
    Staging::Slot<uint32_t> node_id;
    Staging::Slot<int32_t> node_off, feat;
  } a[1 + ORBX_NEW_POINTS_MAX_NEIGHBOURS];
  size_t zstride = 1;
  for (int s = 0; s <= nn; s++) {
    const Kf& K = s ? p->neighbours[s - 1] : p->current;
    const orbx_tri_kf& k = K.kf;
    const size_t n = (size_t)k.n, nnod = (size_t)k.n_nodes;
    if (s && n > zstride) zstride = n;
    a[s].keys = S.in(k.keys_un, n);
    a[s].desc = S.in(k.desc, n * 32);
    a[s].ur = S.in_opt(k.u_right, n);
    a[s].has_mp = s ? S.in_opt(k.has_mp, n) : Staging::Slot<uint8_t>{};  // (the current keyframe's: has_mp1)
    a[s].xy = S.in_opt(K.keys_xy, n * 2);
    a[s].depth = S.in_opt(K.depth, n);
    a[s].mp = s && p->monocular ? S.in_opt(K.mp_pos, n * 3) : Staging::Slot<float>{};
    a[s].node_id = S.in(k.node_id, nnod);
    a[s].node_off = S.in(k.node_off, nnod + 1);
    a[s].feat = S.in(k.feat, nnod ? (size_t)k.node_off[nnod] : 0);
  }
  const auto s_job = S.record<Job>();
  const auto s_nb = S.record<Kf>((size_t)(nn ? nn : 1));
  const auto s_tri = S.record<orbx_tri_problem>((size_t)(nn ? nn : 1));
  const auto o_cnt = S.out<int32_t>(2);
  const auto o_has = S.inout<uint8_t>(p->current.kf.has_mp, n1);
  const auto o_idx = S.out<int32_t>(n1 * 3);
  const auto o_pos = S.out<float>(n1 * 3), o_nrm = S.out<float>(n1 * 3), o_dst = S.out<float>(n1 * 2);
  const auto o_skip = S.out<int32_t>((size_t)nn), o_nm = S.out<int32_t>((size_t)nn);
  const auto o_base = S.out<float>((size_t)nn), o_med = S.out<float>((size_t)nn);
  const size_t npr = probes ? (size_t)nn * n1 : 0;
  const auto o_exit = S.out<uint8_t>(npr);
  const auto o_cos = S.out<float>(npr * 3);
  const auto o_f12 = S.out<float>(probes ? (size_t)nn * 9 : 0);
  const auto o_m12 = S.out<int32_t>(npr);
  const auto d_m12 = S.device_only<int32_t>(probes ? 0 : (size_t)nn * n1);
  const auto d_nm = S.device_only<int32_t>((size_t)(nn ? nn : 1));
  const auto d_pairs = S.device_only<int32_t>(n1 ? n1 : 1);
  const auto d_ctl = S.device_only<int32_t>(4);
  const auto d_pose = S.device_only<Pose>((size_t)nn + 1);
  const auto d_z = S.device_only<float>(p->monocular ? (size_t)(nn ? nn : 1) * zstride : 1);
  cs = S.commit();
  if (cs != ORBX_OK) return cs;

  Job J;
  std::memset(&J, 0, sizeof(J));
  auto view = [&](const Kf& K, int s) {
    Kf v = K;
    v.kf.keys_un = S.dev(a[s].keys);
    v.kf.desc = S.dev(a[s].desc);
    v.kf.u_right = S.dev(a[s].ur);
    v.kf.has_mp = S.dev(a[s].has_mp);
    v.kf.node_id = S.dev(a[s].node_id);
    v.kf.node_off = S.dev(a[s].node_off);
    v.kf.feat = S.dev(a[s].feat);
    v.keys_xy = S.dev(a[s].xy);
    v.depth = S.dev(a[s].depth);
    v.mp_pos = S.dev(a[s].mp);
    return v;
  };
  J.cur = view(p->current, 0);
  J.cur.kf.has_mp = S.dev(o_has);
  J.nb = S.dev(s_nb);
  J.n_nb = nn;
  J.monocular = p->monocular != 0;
  J.raise_after = h->opt.raise_after_neighbour;
  J.zstride = (int)zstride;
  J.ratio_factor = 1.5f * p->scale_factor;
  J.flag = h->flags.dev<const int>();
  J.tri = S.dev(s_tri);
  J.pose = S.dev(d_pose);
  J.zbuf = S.dev(d_z);
  J.match12 = probes ? S.dev(o_m12) : S.dev(d_m12);
  J.nmatches = S.dev(d_nm);
  J.pairs = S.dev(d_pairs);
  J.ctl = S.dev(d_ctl);
  J.n_new = S.dev(o_cnt);
  J.nb_done = S.dev(o_cnt) + 1;
  J.pt_idx = S.dev(o_idx);
  J.pt_pos = S.dev(o_pos), J.pt_normal = S.dev(o_nrm), J.pt_dist = S.dev(o_dst);
  J.nb_skip = S.dev(o_skip), J.nb_nm = S.dev(o_nm);
  J.nb_base = S.dev(o_base), J.nb_med = S.dev(o_med);
  J.has_mp1 = S.dev(o_has);
  J.pr_exit = probes ? S.dev(o_exit) : nullptr;
  J.pr_cos = probes ? S.dev(o_cos) : nullptr;
  J.pr_f12 = probes ? S.dev(o_f12) : nullptr;
  S.fill(s_job, J);
  for (int i = 0; i < nn; i++) {
    const Kf v = view(p->neighbours[i], i + 1);
    S.fill(s_nb, v, (size_t)i);
    orbx_tri_problem T;
    np_tri_pointers(J, i, &T);
    T.kf2 = v.kf;
    S.fill(s_tri, T, (size_t)i);
  }
  int* const mirror = h->flags.as<int>() + 1;
  *mirror = stop && *stop ? 1 : 0;
  hipError_t e = S.upload(Staging::Outputs::zeroed);
  if (e == hipSuccess) e = np_enqueue(J, S.dev(s_job), S.stream());
  if (e == hipSuccess) e = S.download();
  if (e == hipSuccess) {
    if (!stop) {
      e = S.sync();
    } else {  // the device's view of the caller's bool follows it while this thread waits
      for (;;) {
        const int v = *stop ? 1 : 0;
        if (*(volatile int*)mirror != v) *(volatile int*)mirror = v;
        e = hipStreamQuery(S.stream());
        if (e != hipErrorNotReady) break;
        std::this_thread::yield();
      }
      if (e == hipSuccess) e = S.sync();
    }
  }
  *mirror = 0;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return ORBX_ERR_HIP;
  }
  S.fetch(o_cnt, r->n_new, 1);
  *r->neighbours_done = S.host(o_cnt)[1];
  S.fetch(o_has, r->has_mp1, n1);
  S.fetch(o_idx, r->point_idx, n1 * 3);
  S.fetch(o_pos, r->point_pos, n1 * 3);
  S.fetch(o_nrm, r->point_normal, n1 * 3);
  S.fetch(o_dst, r->point_dist, n1 * 2);
  S.fetch(o_skip, r->nb_skip, (size_t)nn);
  S.fetch(o_nm, r->nb_nmatches, (size_t)nn);
  S.fetch(o_base, r->nb_baseline, (size_t)nn);
  S.fetch(o_med, r->nb_median_depth, (size_t)nn);
  h->have_probes = probes;
  if (probes) {
    h->pr_exit.assign(S.host(o_exit), S.host(o_exit) + npr);
    h->pr_cos.assign(S.host(o_cos), S.host(o_cos) + npr * 3);
    h->pr_f12.assign(S.host(o_f12), S.host(o_f12) + (size_t)nn * 9);
    h->pr_m12.assign(S.host(o_m12), S.host(o_m12) + npr);
  }
  return ORBX_OK;
}

}  // namespace

extern "C" {

orbx_status orbx_new_points_create(int device, orbx_new_points** out) {
  if (!out) return ORBX_ERR_ARG;
  *out = nullptr;
  const orbx_status dv = orbx::select_device(device);
  if (dv != ORBX_OK) return dv;
  orbx_new_points* h = new (std::nothrow) orbx_new_points;
  if (!h) return ORBX_ERR_HIP;
  h->device = device;
  if (h->flags.ensure(2 * sizeof(int)) != hipSuccess) {
    (void)hipGetLastError();
    delete h;
    return ORBX_ERR_HIP;
  }
  h->flags.as<int>()[0] = h->flags.as<int>()[1] = 0;
  *out = h;
  return ORBX_OK;
}

orbx_status orbx_new_points_destroy(orbx_new_points* h) {
  if (!h) return ORBX_ERR_ARG;
  (void)hipSetDevice(h->device);
  delete h;
  return ORBX_OK;
}

orbx_status orbx_new_points_stop_flag(orbx_new_points* h, volatile int** flag) {
  if (!h || !flag) return ORBX_ERR_ARG;
  *flag = h->flags.as<int>();
  return ORBX_OK;
}

orbx_status orbx_create_new_map_points(orbx_new_points* h, const orbx_new_points_problem* problem,
                                       const orbx_new_points_result* result) {
  return np_run_host(h, problem, result, nullptr);
}

orbx_status orbx_create_new_map_points_bool(orbx_new_points* h, const orbx_new_points_problem* problem,
                                            const orbx_new_points_result* result, const volatile bool* stop) {
  return np_run_host(h, problem, result, stop);
}

orbx_status orbx_create_new_map_points_device(orbx_new_points* h, const orbx_new_points_problem* p,
                                              const orbx_new_points_result* r, void* stream) {
  if (!h) return ORBX_ERR_ARG;
  const orbx_status cs = np_check_sizes(p);
  if (cs != ORBX_OK) return cs;
  if (!np_result_ok(p, r)) return ORBX_ERR_ARG;
  const int nn = p->n_neighbours, nn1 = nn ? nn : 1;
  const size_t n1 = (size_t)p->current.kf.n;
  size_t zstride = 1;
  for (int i = 0; i < nn; i++)
    if ((size_t)p->neighbours[i].kf.n > zstride) zstride = (size_t)p->neighbours[i].kf.n;
  // one stream-ordered block: job | neighbours | search problems | match12 | nmatches | pairs | ctl | poses | z
  using orbx::scratch_align;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += scratch_align(bytes);
    return o;
  };
  const size_t f_job = take(sizeof(Job)), f_nb = take(sizeof(Kf) * nn1), f_tri = take(sizeof(orbx_tri_problem) * nn1);
  const size_t up_bytes = off;
  const size_t f_m12 = take(sizeof(int32_t) * (nn1 * (n1 ? n1 : 1))), f_nm = take(sizeof(int32_t) * nn1);
  const size_t f_pairs = take(sizeof(int32_t) * (n1 ? n1 : 1)), f_ctl = take(sizeof(int32_t) * 4);
  const size_t f_pose = take(sizeof(Pose) * (nn + 1));
  const size_t f_z = take(sizeof(float) * (p->monocular ? nn1 * zstride : 1));
  hipStream_t st = (hipStream_t)stream;
  std::vector<uint8_t> hostblk(up_bytes, 0);
  return orbx::with_stream_block(off, st, [&](uint8_t* d) {
    Job J;
    std::memset(&J, 0, sizeof(J));
    J.cur = p->current;
    J.cur.kf.has_mp = r->has_mp1;
    J.nb = (const Kf*)(d + f_nb);
    J.n_nb = nn;
    J.monocular = p->monocular != 0;
    J.raise_after = h->opt.raise_after_neighbour;
    J.zstride = (int)zstride;
    J.ratio_factor = 1.5f * p->scale_factor;
    J.flag = h->flags.dev<const int>();
    J.tri = (orbx_tri_problem*)(d + f_tri);
    J.pose = (Pose*)(d + f_pose);
    J.zbuf = (float*)(d + f_z);
    J.match12 = (int32_t*)(d + f_m12);
    J.nmatches = (int32_t*)(d + f_nm);
    J.pairs = (int32_t*)(d + f_pairs);
    J.ctl = (int32_t*)(d + f_ctl);
    J.n_new = r->n_new, J.nb_done = r->neighbours_done, J.pt_idx = r->point_idx;
    J.pt_pos = r->point_pos, J.pt_normal = r->point_normal, J.pt_dist = r->point_dist;
    J.nb_skip = r->nb_skip, J.nb_nm = r->nb_nmatches, J.nb_base = r->nb_baseline, J.nb_med = r->nb_median_depth;
    J.has_mp1 = r->has_mp1;
    std::memcpy(hostblk.data() + f_job, &J, sizeof(J));
    for (int i = 0; i < nn; i++) {
      std::memcpy(hostblk.data() + f_nb + sizeof(Kf) * i, &p->neighbours[i], sizeof(Kf));
      orbx_tri_problem T;
      np_tri_pointers(J, i, &T);
      T.kf2 = p->neighbours[i].kf;
      std::memcpy(hostblk.data() + f_tri + sizeof(T) * i, &T, sizeof(T));
    }
    // (pageable source: the copy is staged before the call returns, so hostblk may go)
    hipError_t e = hipMemcpyAsync(d, hostblk.data(), up_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = np_enqueue(J, (const Job*)(d + f_job), st);
    return e;
  });
}

int orbx_debug_new_points_options(orbx_new_points* h, const orbx_new_points_debug_options* options) {
  if (!h) return ORBX_ERR_ARG;
  h->opt = options ? *options : orbx_new_points_debug_options{-1, 0};
  return ORBX_OK;
}

long long orbx_debug_new_points_probe(orbx_new_points* h, int what, void* dst, size_t cap) {
  if (!h) return ORBX_ERR_ARG;
  if (!h->have_probes) return ORBX_ERR_STATE;
  const void* src;
  size_t bytes;
  switch (what) {
    case ORBX_NP_PROBE_EXIT: src = h->pr_exit.data(), bytes = h->pr_exit.size(); break;
    case ORBX_NP_PROBE_COS: src = h->pr_cos.data(), bytes = h->pr_cos.size() * 4; break;
    case ORBX_NP_PROBE_F12: src = h->pr_f12.data(), bytes = h->pr_f12.size() * 4; break;
    case ORBX_NP_PROBE_MATCH12: src = h->pr_m12.data(), bytes = h->pr_m12.size() * 4; break;
    default: return ORBX_ERR_ARG;
  }
  if (dst && bytes) std::memcpy(dst, src, cap < bytes ? cap : bytes);
  return (long long)bytes;
}

int orbx_debug_new_points_host(const orbx_new_points_problem* p, int neighbour, const int32_t* match12, int32_t* skip,
                               float* baseline, float* median_depth, float F12[9], uint8_t* exit_code, float* cos3,
                               float* pos, float* normal, float* dist) {
  using namespace orbx::cnmp;
  orbx_status cs = np_check_sizes(p);
  if (cs != ORBX_OK) return cs;
  if (neighbour < 0 || neighbour >= p->n_neighbours || !skip || !baseline || !median_depth || !F12) return ORBX_ERR_ARG;
  cs = np_check_host(p);
  if (cs != ORBX_OK) return cs;
  const Kf &K1 = p->current, &K2 = p->neighbours[neighbour];
  Pose P1, P2;
  cn_pose(K1, &P1);
  cn_pose(K2, &P2);
  int n = 0;
  float med = 0.f;
  if (p->monocular && K2.kf.has_mp && K2.mp_pos) {
    std::vector<float> z((size_t)K2.kf.n, 0.f);
    for (int i = 0; i < K2.kf.n; i++)
      if (K2.kf.has_mp[i]) {
        z[i] = cn_depth(P2, K2.mp_pos + 3 * (size_t)i);
        n++;
      }
    const int k = (n - 1) / 2;
    for (int i = 0; i < K2.kf.n && n > 0; i++)
      if (K2.kf.has_mp[i]) {
        const float v = z[i];
        int lt = 0, le = 0;
        for (int j = 0; j < K2.kf.n; j++)
          if (K2.kf.has_mp[j]) {
            lt += z[j] < v;
            le += z[j] <= v;
          }
        if (lt <= k && k < le) med = v;
      }
  }
  *baseline = cn_baseline(P1, P2);
  const int code = cn_gate_code(p->monocular != 0, *baseline, K2.mb, n, med);
  *skip = code;
  *median_depth = p->monocular && code != ORBX_NP_NB_NO_DEPTHS ? med : 0.f;
  for (int k = 0; k < 9; k++) F12[k] = 0.f;
  if (code != ORBX_NP_NB_RAN) return ORBX_OK;
  cn_f12(K1, P1, K2, P2, F12);
  if (!match12) return ORBX_OK;
  if (!exit_code || !cos3 || !pos || !normal || !dist) return ORBX_ERR_ARG;
  const float ratioFactor = 1.5f * p->scale_factor;
  for (int i = 0; i < K1.kf.n; i++) {
    exit_code[i] = ORBX_NP_NONE;
    const int m = match12[i];
    if (m < 0) continue;
    if (m >= K2.kf.n) return ORBX_ERR_ARG;
    float At[16], Vt[16];
    double W[4];
    PairOut o;
    std::memset(&o, 0, sizeof(o));
    const int c = cn_pair(K1, P1, K2, P2, ratioFactor, i, m, At, Vt, W, &o);
    exit_code[i] = (uint8_t)c;
    cos3[3 * i] = o.cosr, cos3[3 * i + 1] = o.cos1, cos3[3 * i + 2] = o.cos2;
    if (c >= ORBX_NP_TRIANGULATED && c <= ORBX_NP_UNPROJECT2) {
      for (int k = 0; k < 3; k++) {
        pos[3 * i + k] = o.X[k];
        normal[3 * i + k] = o.normal[k];
      }
      dist[2 * i] = o.dmin, dist[2 * i + 1] = o.dmax;
    }
  }
  return ORBX_OK;
}

}  // extern "C"

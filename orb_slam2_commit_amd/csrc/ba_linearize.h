// ba_linearize.h -- LocalBundleAdjustment (localba.hip): per-edge errors and robust chi
// (k_ba_errors), linearisation and the point / pose sums (k_ba_linearize, k_ba_point_sum,
// k_ba_cam_sum, k_ba_cam_fin), the point side of the Schur complement (k_ba_point_schur), and the
// fused point-side kernel of the device LM loop (k_ba_lin_schur).
#pragma once
#include "ba_math.h"

namespace orbx {

__device__ inline void edge_error(const BaDev& D, int e, double err[3], double& chi2) {
  const int c = D.ecam[e], p = D.ept[e];
  Quat q = {D.cq[4 * c], D.cq[4 * c + 1], D.cq[4 * c + 2], D.cq[4 * c + 3]};
  const double Xw[3] = {D.X[3 * p], D.X[3 * p + 1], D.X[3 * p + 2]};
  double Pc[3];
  qrot(q, Xw, Pc);
  for (int i = 0; i < 3; i++) Pc[i] += D.ct[3 * c + i];
  const double fx = D.intr[5 * c], fy = D.intr[5 * c + 1], cx = D.intr[5 * c + 2], cy = D.intr[5 * c + 3];
  const double info = D.einfo[e];
  if (!D.est[e]) {
    const double u = Pc[0] / Pc[2] * fx + cx, v = Pc[1] / Pc[2] * fy + cy;
    err[0] = D.eobs[3 * e] - u;
    err[1] = D.eobs[3 * e + 1] - v;
    err[2] = 0;
    chi2 = err[0] * (info * err[0]) + err[1] * (info * err[1]);
  } else {
    const float invz = (float)(1.0 / Pc[2]);
    const float bff = (float)D.intr[5 * c + 4];
    const double u = Pc[0] * invz * fx + cx, v = Pc[1] * invz * fy + cy;
    const double ur = u - (double)(bff * invz);
    err[0] = D.eobs[3 * e] - u;
    err[1] = D.eobs[3 * e + 1] - v;
    err[2] = D.eobs[3 * e + 2] - ur;
    chi2 = err[0] * (info * err[0]) + err[1] * (info * err[1]) + err[2] * (info * err[2]);
  }
}

__device__ inline void huber(double chi, double delta, float dsqr, double rho[3]) {
  if (chi <= dsqr) {
    rho[0] = chi;
    rho[1] = 1.;
    rho[2] = 0.;
  } else {
    const double sq = sqrt(chi);
    rho[0] = 2 * sq * delta - dsqr;
    rho[1] = delta / sq;
    rho[2] = -0.5 * rho[1] / chi;
  }
}

// Returns false where the block did nothing (gated launch, block past the problem): uniform per block.
// coh: the block partial is stored write-through (st_agent) for k_ba_errors_ctl's last block.
template <bool coh = false>
__device__ __forceinline__ bool k_ba_errors_body(const BaDev& D, int recompute, int dst) {
  // recompute == 2: the refresh launch (only while the device LM state asks for it)
  if (recompute == 2 ? !(D.lm && D.lm->refresh) : lm_skip(D)) return false;
  if ((int)blockIdx.x >= D.nbe) return false;  // (a batched grid spans the largest problem)
  const int k = blockIdx.x * LBS + threadIdx.x;
  double chi = 0;
  if (k < D.na) {
    const int e = D.act[k];
    // robust-kernel inputs loaded up front (not behind the eerr stores and the flag's branch)
    const bool rob = D.erobust[e] != 0;
    const double dl = D.edelta[e];
    const float ds = D.edsqr[e];
    double c2;
    if (recompute) {
      double err[3];
      edge_error(D, e, err, c2);
      D.eerr[3 * e] = err[0];
      D.eerr[3 * e + 1] = err[1];
      D.eerr[3 * e + 2] = err[2];
    } else {
      const double info = D.einfo[e];
      c2 = 0;
      for (int i = 0; i < (D.est[e] ? 3 : 2); i++) c2 += D.eerr[3 * e + i] * (info * D.eerr[3 * e + i]);
    }
    chi = c2;
    if (rob) {
      double rho[3];
      huber(c2, dl, ds, rho);
      chi = rho[0];
    }
    // debug hook (ORBX_BA_NAN_TRIAL): the given trial's chi is NaN, i.e. rho is NaN
    if (dst == 1 && k == 0 && D.nan_trial >= 0 && D.lm && D.lm->trials == D.nan_trial)
      chi = __builtin_nan("");
  }
  if (coh) {
    __shared__ double red[LBS / 64];
    const double bs = block_sum1(chi, red);
    if (threadIdx.x == 0) st_agent(D.scal + 8 + dst * D.nbe + blockIdx.x, bs);
    return true;
  }
  block_partial(chi, D.scal + 8 + dst * D.nbe, D.rb_out ? D.rb_out + 8 + dst * D.nbe : nullptr);
  if (D.rb_out && blockIdx.x == 0) {
    // the readback block's other entries (written by earlier launches), then the LM state
    const int n_rb = 8 + 2 * D.nbe + D.nbu;
    for (int i = threadIdx.x; i < n_rb; i += LBS)
      if (i < 8 + dst * D.nbe || i >= 8 + (dst + 1) * D.nbe) D.rb_out[i] = D.scal[i];
    if (D.lm_out) {
      constexpr int kW = sizeof(LmState) / 4;
      static_assert(sizeof(LmState) % 4 == 0, "LmState copied as words");
      if (threadIdx.x < kW)
        reinterpret_cast<uint32_t*>(D.lm_out)[threadIdx.x] = reinterpret_cast<const uint32_t*>(D.lm_copy)[threadIdx.x];
    }
  }
  return true;
}
__global__ __launch_bounds__(LBS) void k_ba_errors(BaDev D, int recompute, int dst) { k_ba_errors_body(D, recompute, dst); }
__global__ __launch_bounds__(LBS) void k_ba_errors_many(const BaDev* __restrict__ Ds, int recompute, int dst) {
  k_ba_errors_body(Ds[blockIdx.z], recompute, dst);
}

// One staged output array of the linearisation: each thread's NV values go to
// LDS, then the block's contiguous NV doubles per position leave with
// coalesced 8-B stores (position k's values land at out[NV * k + j], as
// before); PARTS > 1 stages the block's positions in that many slices so the
// LDS buffer stays at LBS * 21 doubles.
template <int NV, int PARTS, class F>
__device__ __forceinline__ void lin_stage_store(double* sh, double* out, int k0, int nk, bool act, F f) {
  constexpr int PS = LBS / PARTS;
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < PARTS; q++) {
    if (act && t / PS == q) f(sh + NV * (t - q * PS));
    __syncthreads();
    const int n = min(PS, nk - q * PS);
    for (int j = t; j < n * NV; j += LBS) out[NV * ((size_t)k0 + q * PS) + j] = sh[j];
    __syncthreads();
  }
}

// constructQuadraticForm terms of one edge (DIM = 2 mono, 3 stereo); written
// through LDS by the block (positions on fixed cameras get pose terms too:
// nothing reads them).
struct LinTerms {
  double omr[3], W;
};
template <int DIM>
__device__ __forceinline__ LinTerms lin_weights(const BaDev& D, int e) {
  LinTerms T;
  const double info = D.einfo[e];
  const bool rob = D.erobust[e] != 0;
  const double dl = D.edelta[e];
  const float ds = D.edsqr[e];
  T.W = info;
#pragma unroll
  for (int i = 0; i < DIM; i++) T.omr[i] = -info * D.eerr[3 * e + i];
  if (rob) {
    double c2 = 0;
#pragma unroll
    for (int i = 0; i < DIM; i++) c2 += D.eerr[3 * e + i] * (info * D.eerr[3 * e + i]);
    double rho[3];
    huber(c2, dl, ds, rho);
    T.W = rho[1] * info;
#pragma unroll
    for (int i = 0; i < DIM; i++) T.omr[i] *= rho[1];
  }
  return T;
}
template <int DIM>
__device__ __forceinline__ void lin_point_terms(const LinTerms& T, const double* A, double* pc) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    double s = 0;
#pragma unroll
    for (int d = 0; d < DIM; d++) s += A[3 * d + r] * T.omr[d];
    pc[9 + r] = s;
#pragma unroll
    for (int cc = 0; cc < 3; cc++) {
      double h = 0;
#pragma unroll
      for (int d = 0; d < DIM; d++) h += A[3 * d + r] * T.W * A[3 * d + cc];
      pc[3 * r + cc] = h;
    }
  }
}
template <int DIM>
__device__ __forceinline__ void lin_pose_terms(const LinTerms& T, const double* Bm, double* cm) {
  // only the upper triangle is ever summed (k_ba_cam_sum, k_ba_pairs; k_ba_schur_fin mirrors it),
  // so only it is formed and stored: kCmc doubles per position instead of 42
  int j = 0;
#pragma unroll
  for (int r = 0; r < 6; r++) {
    double s = 0;
#pragma unroll
    for (int d = 0; d < DIM; d++) s += Bm[6 * d + r] * T.omr[d];
    cm[21 + r] = s;
#pragma unroll
    for (int cc = r; cc < 6; cc++) {
      double h = 0;
#pragma unroll
      for (int d = 0; d < DIM; d++) h += Bm[6 * d + r] * T.W * Bm[6 * d + cc];
      cm[j++] = h;
    }
  }
}
template <int DIM>
__device__ __forceinline__ void lin_cross_terms(const LinTerms& T, const double* A, const double* Bm, double* hp) {
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int cc = 0; cc < 3; cc++) {
      double h = 0;
#pragma unroll
      for (int d = 0; d < DIM; d++) h += Bm[6 * d + r] * T.W * A[3 * d + cc];
      hp[3 * r + cc] = h;
    }
}

// Jacobians (linearizeOplus, types_six_dof_expmap.h:80-141) and robust weights of edge e at the
// current state: point block A (DIM x 3), pose block Bm (DIM x 6), stereo flag.
struct LinEdge {
  double A[9], Bm[18];
  LinTerms T;
  bool st;
};
__device__ __forceinline__ void lin_edge(const BaDev& D, int e, LinEdge& o) {
  const int c = D.ecam[e], p = D.ept[e];
  Quat q = {D.cq[4 * c], D.cq[4 * c + 1], D.cq[4 * c + 2], D.cq[4 * c + 3]};
  const double Xw[3] = {D.X[3 * p], D.X[3 * p + 1], D.X[3 * p + 2]};
  double Pc[3];
  qrot(q, Xw, Pc);
  for (int i = 0; i < 3; i++) Pc[i] += D.ct[3 * c + i];
  const double x = Pc[0], y = Pc[1], z = Pc[2], z_2 = z * z;
  double R[9];
  qmat(q, R);
  const double fx = D.intr[5 * c], fy = D.intr[5 * c + 1], bf = D.intr[5 * c + 4];
  const bool st = D.est[e];
  double* A = o.A;
  double* Bm = o.Bm;
  for (int i = 0; i < 18; i++) Bm[i] = 0.0;
  if (!st) {
    const double tmp[6] = {fx, 0, -x / z * fx, 0, fy, -y / z * fy};
    for (int r = 0; r < 2; r++)
      for (int cc = 0; cc < 3; cc++)
        A[3 * r + cc] = -1. / z * (tmp[3 * r] * R[cc] + tmp[3 * r + 1] * R[3 + cc] + tmp[3 * r + 2] * R[6 + cc]);
  } else {
    for (int cc = 0; cc < 3; cc++) {
      A[cc] = -fx * R[cc] / z + fx * x * R[6 + cc] / z_2;
      A[3 + cc] = -fy * R[3 + cc] / z + fy * y * R[6 + cc] / z_2;
      A[6 + cc] = A[cc] - bf * R[6 + cc] / z_2;
    }
  }
  Bm[0] = x * y / z_2 * fx;
  Bm[1] = -(1 + (x * x / z_2)) * fx;
  Bm[2] = y / z * fx;
  Bm[3] = -1. / z * fx;
  Bm[4] = 0;
  Bm[5] = x / z_2 * fx;
  Bm[6] = (1 + y * y / z_2) * fy;
  Bm[7] = -x * y / z_2 * fy;
  Bm[8] = -x / z * fy;
  Bm[9] = 0;
  Bm[10] = -1. / z * fy;
  Bm[11] = y / z_2 * fy;
  if (st) {
    Bm[12] = Bm[0] - bf * y / z_2;
    Bm[13] = Bm[1] + bf * x / z_2;
    Bm[14] = Bm[2];
    Bm[15] = Bm[3];
    Bm[16] = 0;
    Bm[17] = Bm[5] - bf / z_2;
  }
  o.st = st;
  o.T = st ? lin_weights<3>(D, e) : lin_weights<2>(D, e);
}

__device__ __forceinline__ void k_ba_linearize_body(const BaDev& D) {
  if (lm_skip_lin(D) || D.fused) return;
  __shared__ double sh[LBS * 21];
  const int k0 = blockIdx.x * LBS, k = k0 + threadIdx.x;
  if (k0 >= D.na) return;  // block-uniform
  const int nk = min(LBS, D.na - k0);
  const bool act = k < D.na;
  const int e = act ? D.act[k] : D.act[k0];
  LinEdge L;
  lin_edge(D, e, L);
  lin_stage_store<12, 1>(sh, D.ptc, k0, nk, act, [&](double* o) {
    if (L.st) lin_point_terms<3>(L.T, L.A, o); else lin_point_terms<2>(L.T, L.A, o);
  });
  lin_stage_store<18, 1>(sh, D.Hpl, k0, nk, act, [&](double* o) {
    if (L.st) lin_cross_terms<3>(L.T, L.A, L.Bm, o); else lin_cross_terms<2>(L.T, L.A, L.Bm, o);
  });
  lin_stage_store<kCmc, 2>(sh, D.cmc, k0, nk, act, [&](double* o) {
    if (L.st) lin_pose_terms<3>(L.T, L.Bm, o); else lin_pose_terms<2>(L.T, L.Bm, o);
  });
}
__global__ __launch_bounds__(LBS) void k_ba_linearize(BaDev D) { k_ba_linearize_body(D); }
__global__ __launch_bounds__(LBS) void k_ba_linearize_many(const BaDev* __restrict__ Ds) {
  k_ba_linearize_body(Ds[blockIdx.z]);
}

__device__ __forceinline__ void k_ba_point_sum_body(const BaDev& D) {
  if (lm_skip_lin(D) || D.fused) return;
  const int i = blockIdx.x * LBS + threadIdx.x;
  if (i >= D.npa) return;
  double h[12];
  for (int j = 0; j < 12; j++) h[j] = 0;
  for (int k = D.pt_off[i]; k < D.pt_off[i + 1]; k++) {
    const double* pc = D.ptc + 12 * (size_t)k;
    for (int j = 0; j < 12; j++) h[j] += pc[j];
  }
  for (int j = 0; j < 9; j++) D.Hll[9 * i + j] = h[j];
  for (int j = 0; j < 3; j++) D.bl[3 * i + j] = h[9 + j];
  D.dmax_p[i] = fmax(fmax(fabs(h[0]), fabs(h[4])), fabs(h[8]));
}
__global__ __launch_bounds__(LBS) void k_ba_point_sum(BaDev D) { k_ba_point_sum_body(D); }
__global__ __launch_bounds__(LBS) void k_ba_point_sum_many(const BaDev* __restrict__ Ds) {
  k_ba_point_sum_body(Ds[blockIdx.z]);
}

// Hpp, bp per pose: grid (pose, chunk); a chunk's threads take its positions
// t, t+kGB, ... ; only the upper triangle (21) + b (6) are summed.  Chunk
// partials -> gpart, summed in chunk order by k_ba_cam_fin.
__device__ __forceinline__ void k_ba_cam_sum_body(const BaDev& D) {
  if (lm_skip_lin(D) || (int)blockIdx.x >= D.nposes || (int)blockIdx.y >= D.gsplit) return;
  __shared__ double red[(kGW + 1) * 27];
  const int ci = blockIdx.x;
  double v[27];
#pragma unroll
  for (int j = 0; j < 27; j++) v[j] = 0;
  int lo, hi;
  chunk_range(D.cam_off[ci], D.cam_off[ci + 1], blockIdx.y, D.gsplit, lo, hi);
  for (int t = lo + threadIdx.x; t < hi; t += kGB) {
    const double* cm = D.cmc + kCmc * (size_t)D.cam_pos[t];
#pragma unroll
    for (int j = 0; j < kCmc; j++) v[j] += cm[j];
  }
  const double* tot = block_sum_fixed<27>(v, red);
  if (threadIdx.x < 27) D.gpart[((size_t)ci * D.gsplit + blockIdx.y) * 27 + threadIdx.x] = tot[threadIdx.x];
}
__global__ __launch_bounds__(kGB) void k_ba_cam_sum(BaDev D) { k_ba_cam_sum_body(D); }
__global__ __launch_bounds__(kGB) void k_ba_cam_sum_many(const BaDev* __restrict__ Ds) {
  k_ba_cam_sum_body(Ds[blockIdx.z]);
}

// One 64-thread block per pose: Hpp (symmetric), bp, max |Hpp_jj|.
__device__ __forceinline__ void k_ba_cam_fin_body(const BaDev& D) {
  if (lm_skip_lin(D) || (int)blockIdx.x >= D.nposes) return;
  __shared__ double tot[27];
  const int ci = blockIdx.x, j = threadIdx.x, S = D.gsplit;
  if (j < 27) {
    double t = 0;
    for (int c = 0; c < S; c++) t += D.gpart[((size_t)ci * S + c) * 27 + j];
    tot[j] = t;
  }
  __syncthreads();
  if (j < 36) {
    int r = j / 6, c = j % 6;
    if (c < r) {
      const int t = r;
      r = c;
      c = t;
    }
    D.Hpp[36 * ci + j] = tot[r * 6 - (r * (r - 1)) / 2 + (c - r)];  // upper-triangle index
  } else if (j < 42) {
    D.bp[6 * ci + (j - 36)] = tot[21 + (j - 36)];
  } else if (j == 42) {
    double m = 0;
    for (int r = 0; r < 6; r++) m = fmax(m, fabs(tot[r * 6 - (r * (r - 1)) / 2]));
    D.dmax_c[ci] = m;
  }
}
__global__ __launch_bounds__(64) void k_ba_cam_fin_many(const BaDev* __restrict__ Ds) {
  k_ba_cam_fin_body(Ds[blockIdx.z]);
}

// One thread per active edge position: D = Hll + lambda I of its point,
// Dinv (stored once per point), BD_e = Hpl_e Dinv, cf_e = Hpl_e Dinv bl.
__device__ __forceinline__ void k_ba_point_schur_body(const BaDev& D, double lambda) {
  if (lm_skip(D) || D.fused == 2 || (D.fused && !lm_skip_lin(D))) return;  // k_ba_lin_schur ran this trial
  lambda = lm_lambda(D, lambda);
  // the block's 256 positions are contiguous: Hpl comes in and BD / cf go out
  // through LDS with coalesced 8-B accesses (per-lane 144-B strides made every
  // load/store instruction touch 64 separate lines)
  __shared__ double sh[LBS * 18];
  __shared__ double scf[LBS * 6];
  const int k0 = blockIdx.x * LBS, t = threadIdx.x, k = k0 + t;
  if (k == 0 && D.nposes == 0) D.scal[2] = 1.0;  // no reduced system to factor
  if (k0 >= D.na) return;  // block-uniform
  const int nk = min(LBS, D.na - k0);
  for (int j = t; j < nk * 18; j += LBS) sh[j] = D.Hpl[18 * (size_t)k0 + j];
  __syncthreads();
  double bdv[18], cfv[6];
  const bool act = k < D.na;
  if (act) {
    const int i = D.pos_pt[k];
    double Dm[9];
    for (int j = 0; j < 9; j++) Dm[j] = D.Hll[9 * i + j];
    Dm[0] += lambda;
    Dm[4] += lambda;
    Dm[8] += lambda;
    double Di[9];
    inv3(Dm, Di);
    if (k == D.pt_off[i])
      for (int j = 0; j < 9; j++) D.Dinv[9 * i + j] = Di[j];
    const double b0 = D.bl[3 * i], b1 = D.bl[3 * i + 1], b2 = D.bl[3 * i + 2];
    double db[3];
    for (int r = 0; r < 3; r++) db[r] = Di[3 * r] * b0 + Di[3 * r + 1] * b1 + Di[3 * r + 2] * b2;
    const double* B1 = sh + 18 * t;
    for (int r = 0; r < 6; r++) {
      for (int c = 0; c < 3; c++) bdv[3 * r + c] = B1[3 * r] * Di[c] + B1[3 * r + 1] * Di[3 + c] + B1[3 * r + 2] * Di[6 + c];
      cfv[r] = B1[3 * r] * db[0] + B1[3 * r + 1] * db[1] + B1[3 * r + 2] * db[2];
    }
  }
  __syncthreads();
  if (act) {
    for (int j = 0; j < 18; j++) sh[18 * t + j] = bdv[j];
    for (int r = 0; r < 6; r++) scf[6 * t + r] = cfv[r];
  }
  __syncthreads();
  // (positions on fixed cameras get values too; nothing reads them)
  for (int j = t; j < nk * 18; j += LBS) D.BD[18 * (size_t)k0 + j] = sh[j];
  for (int j = t; j < nk * 6; j += LBS) D.cf[6 * (size_t)k0 + j] = scf[j];
}
__global__ __launch_bounds__(LBS) void k_ba_point_schur(BaDev D, double lambda) { k_ba_point_schur_body(D, lambda); }
__global__ __launch_bounds__(LBS) void k_ba_point_schur_many(const BaDev* __restrict__ Ds, double lambda) {
  k_ba_point_schur_body(Ds[blockIdx.z], lambda);
}

// ---- the point side of an iteration-start trial in one kernel (device LM, one problem) ----
// k_ba_linearize -> k_ba_point_sum -> k_ba_point_schur fused: block b takes the whole points
// pblk[b] .. pblk[b+1] (positions pt_off[pblk[b]] .. pt_off[pblk[b+1]], fewer than kFuseNT: a
// block's points start inside a kFuseStride-position window and no point has more than
// kFuseMaxDeg positions, checked at intake).  128-thread blocks with 63 KB of LDS: two per CU, so
// a config-4 phase's ~450 blocks are all resident at once.  Per position the same linearisation; the point
// terms stay in LDS and each point's thread sums them in position order (k_ba_point_sum's
// order), then D = Hll + lambda I, D^-1 (once per point) and B D^-1, B D^-1 b_l per position from
// the staged Hpl -- bit-identical to the three kernels, without their global round trips.
constexpr int kFuseNT = 128, kFuseStride = 96, kFuseMaxDeg = 32;
// posepart (per fused block and pose, the pose terms summed in the kernel) only up to this many
// free poses: the block's per-pose position masks, one 64-bit word per wave and pose, share the
// kernel's free LDS with the staged pose terms (static_assert at the LDS layout)
constexpr int kPosePartMaxPoses = 256;
// n (even) doubles between 16-B aligned arrays, one 16-B pair per thread and step (half the
// iterations of 8-B copies: these LDS <-> global loops are a block's tail)
typedef double dpair_t __attribute__((ext_vector_type(2)));
template <int NT>
__device__ __forceinline__ void copy_pairs(double* __restrict__ dst, const double* __restrict__ src, int n, int t) {
  dpair_t* d = reinterpret_cast<dpair_t*>(dst);
  const dpair_t* q = reinterpret_cast<const dpair_t*>(src);
  for (int j = t; j < n / 2; j += NT) d[j] = q[j];
}
// Phase probe (build with -DORBX_LS_PROBE only; tools/ls_probe.py): s_memtime of thread 0 of every
// k_ba_lin_schur block at six points of the last launch, 8 words per block
#ifdef ORBX_LS_PROBE
__device__ unsigned long long g_ls_probe[1024 * 8];
#define LS_TS(k)                                                                                  \
  do {                                                                                            \
    if (threadIdx.x == 0 && blockIdx.x < 1024) g_ls_probe[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define LS_TS(k)
#endif
static_assert(kFuseStride - 1 + kFuseMaxDeg <= kFuseNT, "a fused block's positions fit its threads");
__device__ __forceinline__ void k_ba_lin_schur_body(const BaDev& D) {
  if (!D.fused || lm_skip(D) || (int)blockIdx.x >= D.nbf) return;
  // fused == 2: the trials that do not relinearise (a rejected step's new lambda) also come here,
  // for k_ba_point_schur's part: the staged Hpl, D = Hll + lambda I, D^-1 b_l (same bits)
  const bool lin = !lm_skip_lin(D);
  if (!lin && D.fused != 2) return;
  constexpr int NT = kFuseNT;
  extern __shared__ __attribute__((aligned(16))) double fsm[];
  double* sptc = fsm;                // NT x 12 point terms; then with sbuf: BD (18) | cf (6) staging
  double* sbuf = sptc + NT * 12;     // NT x 21; with sdi (before the point sums): the 27 pose terms
  double* sdi = sbuf + NT * 21;      // NT x 12: per point D^-1 (9) and D^-1 b_l (3)
  double* shpl = sdi + NT * 12;      // NT x 18
  double* sout = sptc;               // NT x 24 over sptc + sbuf once the point sums are done
  static_assert(12 + 1 + kCmc <= 12 + 21 + 12, "the pose-term staging fits sbuf + sdi");
  // posepart: NT x kCmc pose terms, then nposes x (NT / 64) mask words, in sbuf + sdi (per thread:
  // kCmc + nposes / 64 doubles of the 21 + 12)
  static_assert(kPosePartMaxPoses % 64 == 0 && kCmc + kPosePartMaxPoses / 64 <= 21 + 12,
                "posepart's staged pose terms and per-pose masks fit sbuf + sdi");
  const int b = blockIdx.x, t = threadIdx.x;
  const int p0 = D.pblk[b], p1 = D.pblk[b + 1];
  const int k0 = D.pt_off[p0], nk = D.pt_off[p1] - k0, npt = p1 - p0;
  if (nk <= 0) return;  // block-uniform
  const double lambda = lm_lambda(D, 0.0);
  const bool act = t < nk;
  const int k = k0 + (act ? t : 0);
  LS_TS(0);
  if (!lin) {
    copy_pairs<NT>(shpl, D.Hpl + 18 * (size_t)k0, nk * 18, t);  // (18 k0 doubles: 16-B aligned)
    if (t < npt) {
      const int i = p0 + t;
      double Dm[9];
      for (int j = 0; j < 9; j++) Dm[j] = D.Hll[9 * i + j];
      Dm[0] += lambda;
      Dm[4] += lambda;
      Dm[8] += lambda;
      double Di[9];
      inv3(Dm, Di);
      for (int j = 0; j < 9; j++) D.Dinv[9 * i + j] = Di[j];
      const double b0 = D.bl[3 * i], b1 = D.bl[3 * i + 1], b2 = D.bl[3 * i + 2];
      for (int r = 0; r < 3; r++) sdi[12 * t + 9 + r] = Di[3 * r] * b0 + Di[3 * r + 1] * b1 + Di[3 * r + 2] * b2;
      for (int j = 0; j < 9; j++) sdi[12 * t + j] = Di[j];
    }
  } else {
  LinEdge L;
  lin_edge(D, D.act[k], L);
  if (act) {
    if (L.st) {
      lin_point_terms<3>(L.T, L.A, sptc + 12 * t);
      lin_cross_terms<3>(L.T, L.A, L.Bm, shpl + 18 * t);
    } else {
      lin_point_terms<2>(L.T, L.A, sptc + 12 * t);
      lin_cross_terms<2>(L.T, L.A, L.Bm, shpl + 18 * t);
    }
  }
  LS_TS(1);
  // the 27 pose terms of every position out through LDS in one pass (sbuf + sdi, free until the
  // point sums) and 16-B pair stores; the staging starts at the global block's parity (27 k0 may be
  // odd), so the LDS and the global pairs are aligned alike
  double cm[kCmc];
  if (L.st) lin_pose_terms<3>(L.T, L.Bm, cm); else lin_pose_terms<2>(L.T, L.Bm, cm);
  if (D.posepart && D.fused != 3) {
    // per pose, the block's positions on it summed in position order (the rhs blocks of k_ba_pairs
    // then add the fused blocks' sums in block order): one nposes x kCmc record per block instead
    // of kCmc doubles per position.  Pose c's positions = the set bits of each wave's ballot,
    // walked in ascending order.
    double* scm = sbuf;                                             // NT x kCmc
    uint64_t* pm = reinterpret_cast<uint64_t*>(sbuf + NT * kCmc);   // nposes x (NT / 64) masks
    const int pc = act ? D.pcam[k] : -1;
    if (act) {
#pragma unroll
      for (int j = 0; j < kCmc; j++) scm[kCmc * t + j] = cm[j];
    }
    const int np = D.nposes;
    for (int c = 0; c < np; c++) {
      const uint64_t m = __ballot(pc == c);
      if ((t & 63) == 0) pm[(NT / 64) * c + (t >> 6)] = m;
    }
    __syncthreads();
    double* dst = D.gpose + (size_t)b * np * kCmc;
    for (int it = t; it < np * kCmc; it += NT) {
      const int c = it / kCmc, j = it - c * kCmc;
      double acc = 0.0;
#pragma unroll
      for (int w = 0; w < NT / 64; w++) {
        uint64_t m = pm[(NT / 64) * c + w];
        while (m) {
          acc += scm[kCmc * (64 * w + __builtin_ctzll(m)) + j];
          m &= m - 1;
        }
      }
      dst[it] = acc;
    }
    __syncthreads();  // (sbuf / sdi are written again below)
  } else {
    const int par = (int)((kCmc * (size_t)k0) & 1), n = nk * kCmc;
    double* scm = sbuf + par;
    if (act) {
#pragma unroll
      for (int j = 0; j < kCmc; j++) scm[kCmc * t + j] = cm[j];
    }
    __syncthreads();
    double* dst = D.cmc + kCmc * (size_t)k0;
    if (par && t == 0) dst[0] = scm[0];
    copy_pairs<NT>(dst + par, scm + par, (n - par) & ~1, t);
    if (((n - par) & 1) && t == NT - 1) dst[n - 1] = scm[n - 1];
    __syncthreads();  // (sbuf / sdi are written again below)
  }
  LS_TS(2);
  copy_pairs<NT>(D.Hpl + 18 * (size_t)k0, shpl, nk * 18, t);
  // point sums (k_ba_point_sum's order), D^-1 and D^-1 b_l once per point
  if (t < npt) {
    const int i = p0 + t;
    const int a = D.pt_off[i] - k0, e = D.pt_off[i + 1] - k0;
    double h[12];
    for (int j = 0; j < 12; j++) h[j] = 0;
    for (int kk = a; kk < e; kk++)
      for (int j = 0; j < 12; j++) h[j] += sptc[12 * kk + j];
    for (int j = 0; j < 9; j++) D.Hll[9 * i + j] = h[j];
    for (int j = 0; j < 3; j++) D.bl[3 * i + j] = h[9 + j];
    D.dmax_p[i] = fmax(fmax(fabs(h[0]), fabs(h[4])), fabs(h[8]));
    if (D.fused == 3) return;  // (a phase's entry linearisation: no lambda yet, no Schur terms)
    double Dm[9];
    for (int j = 0; j < 9; j++) Dm[j] = h[j];
    Dm[0] += lambda;
    Dm[4] += lambda;
    Dm[8] += lambda;
    double Di[9];
    inv3(Dm, Di);
    for (int j = 0; j < 9; j++) D.Dinv[9 * i + j] = Di[j];
    const double b0 = h[9], b1 = h[10], b2 = h[11];
    for (int r = 0; r < 3; r++) sdi[12 * t + 9 + r] = Di[3 * r] * b0 + Di[3 * r + 1] * b1 + Di[3 * r + 2] * b2;
    for (int j = 0; j < 9; j++) sdi[12 * t + j] = Di[j];
  }
  }  // lin
  if (D.fused == 3) return;  // block-uniform
  LS_TS(3);
  __syncthreads();
  LS_TS(4);
  if (act) {
    const double* Di = sdi + 12 * (D.pos_pt[k] - p0);
    const double* db = Di + 9;
    const double* B1 = shpl + 18 * t;
    for (int r = 0; r < 6; r++) {
      for (int c = 0; c < 3; c++)
        sout[18 * t + 3 * r + c] = B1[3 * r] * Di[c] + B1[3 * r + 1] * Di[3 + c] + B1[3 * r + 2] * Di[6 + c];
      sout[18 * NT + 6 * t + r] = B1[3 * r] * db[0] + B1[3 * r + 1] * db[1] + B1[3 * r + 2] * db[2];
    }
  }
  __syncthreads();
  if (!D.bdfold) copy_pairs<NT>(D.BD + 18 * (size_t)k0, sout, nk * 18, t);
  copy_pairs<NT>(D.cf + 6 * (size_t)k0, sout + 18 * NT, nk * 6, t);
  LS_TS(5);
}
__global__ __launch_bounds__(kFuseNT) void k_ba_lin_schur(BaDev D) { k_ba_lin_schur_body(D); }
__global__ __launch_bounds__(kFuseNT) void k_ba_lin_schur_many(const BaDev* __restrict__ Ds) {
  k_ba_lin_schur_body(Ds[blockIdx.z]);
}
constexpr size_t kFuseSmem = (size_t)kFuseNT * (12 + 21 + 18 + 12) * sizeof(double);

// Per phase: pblk[b] = the first active point whose first position is >= b * kFuseStride (block b
// then ends where block b+1's first point starts); pblk[nbf] = npa.  One thread per point, run by the
// pair-table launch's extra blocks.
__device__ __forceinline__ void pblk_body(const BaDev& D, int b) {
  const int p = b * LBS + threadIdx.x;
  if (p > D.npa) return;
  const int cur = p < D.npa ? D.pt_off[p] / kFuseStride : D.nbf;
  const int prev = p == 0 ? -1 : D.pt_off[p - 1] / kFuseStride;
  for (int q = prev + 1; q <= min(cur, D.nbf); q++) D.pblk[q] = p;
}

}  // namespace orbx

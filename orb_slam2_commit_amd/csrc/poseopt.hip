// poseopt.hip -- Optimizer::PoseOptimization (src/Optimizer.cc:287-528), one
// block per frame, the whole four-round g2o Levenberg schedule on the device.
//
// Per frame the problem is a single 6-DoF vertex with n ~ 10^2..10^3 unary
// edges (EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose, Huber),
// so the unit of parallelism is the frame batch: a block per frame keeps the
// LM state in LDS and never returns to the host between rounds, trials or
// iterations.  Inside a block the per-edge work (errors, Jacobians, the 27
// quadratic-form terms) is spread over the threads; the sums that g2o forms
// in edge insertion order (activeRobustChi2, buildSystem's H and b) are then
// taken in exactly that order, one FP64 chain per H/b entry on its own lane,
// from contiguous scratch rows.  With the deterministic sin/cos of
// SE3Quat::exp and the same Eigen-LDLT restatement and Levenberg step as the
// oracle (oracle/poseopt.cpp; both in orbx_lm.h, shared with optsim3.hip), the
// GPU reproduces the oracle bit for bit: pose, outlier flags, return value and
// per-round iteration counts.
//
// Bound: latency (dependent FP64 chains of length n per LM iteration, ~10
// cycles per link); throughput comes from thousands of frames in flight.
// Algorithmic bytes per LM trial: 28 B of edge input + 24 B stored error +
// 8 B chi term per active edge, + 216 B of quadratic-form terms written and
// read once per iteration.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "orbx_device.h"
#include "orbx_scratch.h"
#include "orbx_internal.h"
#include "orbx_lm.h"

namespace orbx {
namespace pose {

using namespace lm;  // Quat, qmul, qrot, qmat, mat2q, qnormalize, ldlt<N>, lds_chain, the Levenberg Step

constexpr int PBS = 256;
constexpr int kRow = 32;  // scratch doubles per edge: 27 terms | err[3] | chi term | pad

struct SE3 {
  Quat q;
  double t[3];
};

// SE3Quat::exp(update), types/se3quat.h:223-257 (then operator* with T)
__device__ __forceinline__ SE3 se3_exp(const double u[6]) {
  const double w[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]};
  const double theta = __builtin_sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double O[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double O2[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) O2[3 * r + c] = O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c] + O[3 * r + 2] * O[6 + c];
  double R[9], V[9];
  if (theta < 0.00001) {
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = ((i % 4) == 0 ? 1.0 : 0.0) + O[i] + O2[i];
#pragma unroll
    for (int i = 0; i < 9; i++) V[i] = R[i];
  } else {
    double s, c;
    sincos_d(theta, &s, &c);
    const double a = s / theta, b = (1 - c) / (theta * theta), d = (theta - s) / (theta * theta * theta);
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const double I = (i % 4) == 0 ? 1.0 : 0.0;
      R[i] = I + a * O[i] + b * O2[i];
      V[i] = I + b * O[i] + d * O2[i];
    }
  }
  SE3 T;
  T.q = mat2q(R);
#pragma unroll
  for (int r = 0; r < 3; r++) T.t[r] = V[3 * r] * up[0] + V[3 * r + 1] * up[1] + V[3 * r + 2] * up[2];
  qnormalize(T.q);
  return T;
}
__device__ __forceinline__ SE3 se3_mul(const SE3& a, const SE3& b) {
  SE3 r = a;
  double rt[3];
  qrot(a.q, b.t, rt);
#pragma unroll
  for (int i = 0; i < 3; i++) r.t[i] += rt[i];
  r.q = qmul(a.q, b.q);
  qnormalize(r.q);
  return r;
}

struct PoseDev {
  orbx_pose_problem p;
  double* scratch;  // n x kRow doubles
  int* act;         // n: active edge ids in insertion order
};

struct Edge {
  bool stereo;
  double obs[3], X[3], info;
};

__device__ __forceinline__ Edge load_edge(const orbx_pose_problem& P, int i) {
  Edge e;
  e.stereo = P.obs[3 * i + 2] >= 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    e.obs[k] = P.obs[3 * i + k];
    e.X[k] = P.Xw[3 * i + k];
  }
  e.info = P.inv_sigma2[i];
  return e;
}

__device__ __forceinline__ void edge_error(const SE3& T, const orbx_pose_problem& P, const Edge& e, double err[3]) {
  double Pc[3];
  qrot(T.q, e.X, Pc);
#pragma unroll
  for (int i = 0; i < 3; i++) Pc[i] += T.t[i];
  const double fx = P.fx, fy = P.fy, cx = P.cx, cy = P.cy;
  if (!e.stereo) {
    const double u = Pc[0] / Pc[2] * fx + cx, v = Pc[1] / Pc[2] * fy + cy;
    err[0] = e.obs[0] - u;
    err[1] = e.obs[1] - v;
    err[2] = 0;
  } else {
    const float invz = (float)(1.0 / Pc[2]);
    const double u = Pc[0] * invz * fx + cx, v = Pc[1] * invz * fy + cy;
    const double ur = u - (double)P.bf * invz;
    err[0] = e.obs[0] - u;
    err[1] = e.obs[1] - v;
    err[2] = e.obs[2] - ur;
  }
}

__device__ __forceinline__ double chi2_of(const Edge& e, const double err[3]) {
  double s = err[0] * (e.info * err[0]);
  s += err[1] * (e.info * err[1]);
  if (e.stereo) s += err[2] * (e.info * err[2]);
  return s;
}

__device__ __forceinline__ void huber(bool stereo, double chi, double rho[3]) {
  const float dm = __builtin_sqrtf(5.991f), ds = __builtin_sqrtf(7.815f);
  const double delta = stereo ? ds : dm;
  const float dsqr = (float)(delta * delta);
  if (chi <= dsqr) {
    rho[0] = chi;
    rho[1] = 1.;
    rho[2] = 0.;
  } else {
    const double sq = __builtin_sqrt(chi);
    rho[0] = 2 * sq * delta - dsqr;
    rho[1] = delta / sq;
    rho[2] = -0.5 * rho[1] / chi;
  }
}

__device__ __forceinline__ void jacobian(const SE3& T, const orbx_pose_problem& P, const Edge& e, double J[18]) {
  double Pc[3];
  qrot(T.q, e.X, Pc);
#pragma unroll
  for (int i = 0; i < 3; i++) Pc[i] += T.t[i];
  const double fx = P.fx, fy = P.fy, bf = P.bf;
  const double x = Pc[0], y = Pc[1], iz = 1.0 / Pc[2], iz2 = iz * iz;
  J[0] = x * y * iz2 * fx;
  J[1] = -(1 + (x * x * iz2)) * fx;
  J[2] = y * iz * fx;
  J[3] = -iz * fx;
  J[4] = 0;
  J[5] = x * iz2 * fx;
  J[6] = (1 + y * y * iz2) * fy;
  J[7] = -x * y * iz2 * fy;
  J[8] = -x * iz * fy;
  J[9] = 0;
  J[10] = -iz * fy;
  J[11] = y * iz2 * fy;
  J[12] = J[0] - bf * y * iz2;
  J[13] = J[1] + bf * x * iz2;
  J[14] = J[2];
  J[15] = J[3];
  J[16] = 0;
  J[17] = J[5] - bf * iz2;
}

// LDS staging of the per-edge terms for the insertion-order sums: a chunk of kCh edges' 21 H
// (upper) + 6 b terms + the chi term at an odd row stride (kTs: lanes of the summing wave read
// consecutive doubles; the writers' 29-double stride spreads over the banks), summed chunk by
// chunk by one lane per entry.  The sums used to read the rows back from global scratch, 8 loads
// in flight per lane: ~700 cycles per 8 links of the chain.
constexpr int kCh = PBS;
constexpr int kTerm = 28, kTs = 29;
constexpr int kChiCh = kCh * kTs;  // chi terms per trial pass (one double each)

struct Shared {
  SE3 T, T0, bak;
  double H[36], b[6], x[6];
  Step lm;  // lambda, ni, currentChi, iniChi, rho, qmax, nBad (orbx_lm.h)
  int ok2, go, term, robust, nbad_cls;
  int scan[PBS / 64];
};

// Phase probe (build with -DORBX_POSE_PROBE only): s_memtime ticks per phase of each block, taken
// by thread 0 after the phase's closing barrier, into a host-provided buffer of 16 words per block.
#ifdef ORBX_POSE_PROBE
__device__ unsigned long long* pose_probe_buf;
#define POSE_TS(k)                                                    \
  do {                                                                \
    if (tid == 0) {                                                   \
      const unsigned long long t_ = __builtin_amdgcn_s_memtime();     \
      pacc[k] += t_ - plast;                                          \
      plast = t_;                                                     \
    }                                                                 \
  } while (0)
#else
#define POSE_TS(k)
#endif

__global__ __launch_bounds__(PBS) void k_pose_optimization(const PoseDev* __restrict__ probs) {
  __shared__ Shared S;
  __shared__ double sterm[kCh * kTs];
#ifdef ORBX_POSE_PROBE
  unsigned long long pacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, plast = __builtin_amdgcn_s_memtime();
#endif
  const PoseDev& D = probs[blockIdx.x];
  const orbx_pose_problem& P = D.p;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n = P.n_dev ? min(max(*P.n_dev, 0), P.n) : P.n;  // device-sized: P.n is the capacity
  double* scr = D.scratch;
  int* act = D.act;
  const float* Tin = P.Tcw_dev ? P.Tcw_dev : P.Tcw;

  for (int i = tid; i < n; i += PBS) P.outlier[i] = 0;
  if (tid < 16) P.Tcw_out[tid] = Tin[tid];
  if (P.iterations && tid < 4) P.iterations[tid] = 0;
  if (n < 3) {  // nInitialCorrespondences < 3: return 0, pose untouched
    if (tid == 0) *P.ngood = 0;
    return;
  }
  if (tid == 0) {  // Converter::toSE3Quat(pFrame->mTcw)
    const float* T = Tin;
    const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    S.T0.q = mat2q(R);
    qnormalize(S.T0.q);
    S.T0.t[0] = T[3];
    S.T0.t[1] = T[7];
    S.T0.t[2] = T[11];
    S.robust = 1;
  }
  __syncthreads();
  int nBad = 0;
  for (int it = 0; it < 4; it++) {
    // ---- initializeOptimization(0): active = level-0 edges, insertion order ----
    if (tid == 0) S.T = S.T0;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += PBS) {
      const int i = c0 + tid;
      compact_chunk<PBS>(i < n && !P.outlier[i], S.scan, base, [&](int slot) { act[slot] = i; });
    }
    const int nact = base;
    __threadfence_block();
    __syncthreads();
    POSE_TS(0);
    int its = 0;
    if (nact > 0) {
      for (int iter = 0; iter < 10; iter++) {
        its++;
        // computeActiveErrors + activeRobustChi2 (currentChi) and buildSystem's terms, a chunk of
        // kCh active edges at a time into LDS, each summed in insertion order by its own lane
        const bool robust = S.robust;
        const SE3 T = S.T;
        double acc = 0.0;  // wave 0, lanes 0..27: H upper (0..20), b (21..26, -= terms), chi (27)
        for (int c0 = 0; c0 < nact; c0 += kCh) {
          const int k = c0 + tid;
          if (k < nact) {
            const int i = act[k];
            const Edge e = load_edge(P, i);
            double err[3];
            edge_error(T, P, e, err);
            double* row = scr + (size_t)k * kRow;  // errors kept for the outlier pass
            row[27] = err[0];
            row[28] = err[1];
            row[29] = err[2];
            double* tr = sterm + tid * kTs;
            const double c = chi2_of(e, err);
            double rho[3];
            if (robust) huber(e.stereo, c, rho);
            tr[27] = robust ? rho[0] : c;
            // buildSystem terms (linearizeOplus + constructQuadraticForm)
            double J[18];
            jacobian(T, P, e, J);
            const int Dm = e.stereo ? 3 : 2;
            double w = e.info, r1 = 1.0;
            if (robust) {
              r1 = rho[1];
              w = rho[1] * e.info;
            }
            int q = 0;
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
              for (int cc = r; cc < 6; cc++) {
                double sv = (J[r] * w) * J[cc];
                sv = sv + (J[6 + r] * w) * J[6 + cc];
                if (Dm == 3) sv = sv + (J[12 + r] * w) * J[12 + cc];
                tr[q++] = sv;
              }
#pragma unroll
            for (int r = 0; r < 6; r++) {
              double sv = ((r1 * J[r]) * e.info) * err[0];
              sv = sv + ((r1 * J[6 + r]) * e.info) * err[1];
              if (Dm == 3) sv = sv + ((r1 * J[12 + r]) * e.info) * err[2];
              tr[21 + r] = sv;
            }
          }
          __syncthreads();
          POSE_TS(1);
          if (wid == 0 && lane < kTerm)
            acc = lds_chain(sterm + lane, min(kCh, nact - c0), kTs, acc, lane >= 21 && lane < 27);
          __syncthreads();
          POSE_TS(2);
        }
        if (wid == 0 && lane < kTerm) {
          if (lane < 21) {
            int r, c;
            tri_rc<6>(lane, r, c);
            S.H[6 * r + c] = acc;
            S.H[6 * c + r] = acc;
          } else if (lane < 27) {
            S.b[lane - 21] = acc;
          } else {
            S.lm.currentChi = acc;
            S.lm.iniChi = acc;
          }
        }
        __syncthreads();
        POSE_TS(2);
        if (tid == 0) {
          if (iter == 0) start(S.lm, lambda_init<6>(S.H));
          S.lm.qmax = 0;
        }
        __syncthreads();
        POSE_TS(3);
        // ---- trials ----
        for (;;) {
          if (tid == 0) {
            S.bak = S.T;
            double Hd[36];  // registers: every index static
#pragma unroll
            for (int j = 0; j < 36; j++) Hd[j] = S.H[j];
#pragma unroll
            for (int j = 0; j < 6; j++) Hd[7 * j] += S.lm.lambda;
            const bool ok2 = ldlt<6>(Hd, S.b, S.x);
            S.ok2 = ok2;
            POSE_TS(9);
            if (ok2) S.T = se3_mul(se3_exp(S.x), S.T);
          }
          __syncthreads();
          POSE_TS(4);
          double tempChi = 0.0;  // thread 0: activeRobustChi2 at the trial pose, insertion order
          {
            const SE3 Tt = S.T;
            const bool rb = S.robust;
            for (int c0 = 0; c0 < nact; c0 += kChiCh) {
              for (int k = c0 + tid; k < min(nact, c0 + kChiCh); k += PBS) {
                const int i = act[k];
                const Edge e = load_edge(P, i);
                double err[3];
                edge_error(Tt, P, e, err);
                double* row = scr + (size_t)k * kRow;
                row[27] = err[0];
                row[28] = err[1];
                row[29] = err[2];
                const double c = chi2_of(e, err);
                double rho[3];
                if (rb) huber(e.stereo, c, rho);
                sterm[k - c0] = rb ? rho[0] : c;
              }
              __syncthreads();
              POSE_TS(5);
              if (tid == 0) tempChi = lds_chain(sterm, min(kChiCh, nact - c0), 1, tempChi, false);
              __syncthreads();
              POSE_TS(6);
            }
          }
          if (tid == 0) {
            const bool ok2 = S.ok2;
            double scale = 0.0;
            if (ok2)
              for (int j = 0; j < 6; j++) scale += S.x[j] * (S.lm.lambda * S.x[j] + S.b[j]);
            const Verdict v = trial<Cube::kProduct>(S.lm, tempChi, scale, ok2);
            if (!v.accept) S.T = S.bak;  // pop
            S.go = v.go;
          }
          __syncthreads();
          POSE_TS(7);
          if (!S.go) break;
        }
        if (tid == 0) S.term = iteration_end(S.lm);
        __syncthreads();
        POSE_TS(7);
        if (S.term) break;
      }
    }
    if (P.iterations && tid == 0) P.iterations[it] = its;
    // ---- outlier classification, src/Optimizer.cc:433-497 ----
    // stored errors of active edges sit in the scratch rows of their active position
    if (tid == 0) S.nbad_cls = 0;
    __syncthreads();
    {
      const SE3 T = S.T;
      // map edge -> active position: act[] is ascending, binary search
      int cnt = 0;
      for (int i = tid; i < n; i += PBS) {
        const Edge e = load_edge(P, i);
        double err[3];
        if (P.outlier[i]) {
          edge_error(T, P, e, err);  // e->computeError()
        } else {
          int lo = 0, hi = nact;
          while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (act[m] < i) lo = m + 1; else hi = m;
          }
          const double* row = scr + (size_t)lo * kRow;
          err[0] = row[27];
          err[1] = row[28];
          err[2] = row[29];
        }
        const float chi2 = (float)chi2_of(e, err);
        const bool bad = chi2 > (e.stereo ? 7.815f : 5.991f);
        cnt += bad;
        // written after every thread has read the old flags (barrier below)
        scr[(size_t)i * kRow + 31] = bad ? 1.0 : 0.0;
      }
      atomicAdd(&S.nbad_cls, cnt);
    }
    __threadfence_block();
    __syncthreads();
    POSE_TS(8);
    for (int i = tid; i < n; i += PBS) P.outlier[i] = scr[(size_t)i * kRow + 31] != 0.0 ? 1 : 0;
    nBad = S.nbad_cls;
    if (it == 2 && tid == 0) S.robust = 0;
    __threadfence_block();
    __syncthreads();
    POSE_TS(8);
    if (n < 10) break;
  }
#ifdef ORBX_POSE_PROBE
  if (tid == 0 && pose_probe_buf)
    for (int k = 0; k < 10; k++) pose_probe_buf[(size_t)blockIdx.x * 16 + k] = pacc[k];
#endif
  if (tid == 0) {
    double R[9];
    qmat(S.T.q, R);
    for (int r = 0; r < 3; r++) {
      for (int k = 0; k < 3; k++) P.Tcw_out[4 * r + k] = (float)R[3 * r + k];
      P.Tcw_out[4 * r + 3] = (float)S.T.t[r];
    }
    P.Tcw_out[12] = P.Tcw_out[13] = P.Tcw_out[14] = 0.0f;
    P.Tcw_out[15] = 1.0f;
    *P.ngood = n - nBad;
  }
}

}  // namespace pose
}  // namespace orbx

#ifdef ORBX_POSE_PROBE
extern "C" int orbx_debug_pose_probe(void* d_buf) {  // device buffer of 16 u64 per block, or NULL
  unsigned long long* p = (unsigned long long*)d_buf;
  return hipMemcpyToSymbol(HIP_SYMBOL(orbx::pose::pose_probe_buf), &p, sizeof(p)) == hipSuccess ? 0 : -3;
}
#endif

// ------------------------------------------------------------------ C ABI
namespace {

orbx_status pose_check(const orbx_pose_problem& p) {
  if (p.n < 0) return ORBX_ERR_ARG;
  if (!p.Tcw_out || !p.ngood) return ORBX_ERR_ARG;
  if (p.n > 0 && (!p.obs || !p.Xw || !p.inv_sigma2 || !p.outlier)) return ORBX_ERR_ARG;
  return ORBX_OK;
}

}  // namespace

extern "C" orbx_status orbx_pose_optimization(const orbx_pose_problem* p, int device) {
  if (!p) return ORBX_ERR_ARG;
  const orbx_status chk = pose_check(*p);
  if (chk != ORBX_OK) return chk;
  if (p->n_dev || p->Tcw_dev) return ORBX_ERR_ARG;  // device batches only
  const orbx_status dv = orbx::select_device(device);
  if (dv != ORBX_OK) return dv;
  using orbx::Staging;
  using orbx::pose::PoseDev;
  const size_t n = (size_t)p->n;
  Staging S(device);  // pooled lease: no per-call allocation (orbx_scratch.h)
  const auto s_obs = S.in(p->obs, n * 3), s_X = S.in(p->Xw, n * 3), s_s2 = S.in(p->inv_sigma2, n);
  const auto s_dev = S.record<PoseDev>();
  const auto s_Tout = S.out<float>(16);
  const auto s_out = S.out<uint8_t>(n);
  const auto s_ng = S.out<int32_t>(1), s_it = S.out<int32_t>(4);
  const auto s_scr = S.device_only<double>(n * orbx::pose::kRow);
  const auto s_act = S.device_only<int>(n);
  const orbx_status cs = S.commit();
  if (cs != ORBX_OK) return cs;
  PoseDev pd;
  pd.p = *p;
  pd.p.obs = S.dev(s_obs);
  pd.p.Xw = S.dev(s_X);
  pd.p.inv_sigma2 = S.dev(s_s2);
  pd.p.Tcw_out = S.dev(s_Tout);
  pd.p.outlier = S.dev(s_out);
  pd.p.ngood = S.dev(s_ng);
  pd.p.iterations = S.dev(s_it);
  pd.scratch = S.dev(s_scr);
  pd.act = S.dev(s_act);
  S.fill(s_dev, pd);
  hipError_t e = S.upload(Staging::Outputs::zeroed);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(orbx::pose::k_pose_optimization, dim3(1), dim3(orbx::pose::PBS), 0, S.stream(),
                       (const PoseDev*)S.dev(s_dev));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = S.download();
  if (e == hipSuccess) e = S.sync();
  if (e != hipSuccess) return ORBX_ERR_HIP;
  S.fetch(s_Tout, p->Tcw_out, 16);
  S.fetch(s_out, p->outlier, n);
  S.fetch(s_ng, p->ngood, 1);
  S.fetch(s_it, p->iterations, 4);
  return ORBX_OK;
}

extern "C" orbx_status orbx_pose_optimization_device(const orbx_pose_problem* problems, int n, void* stream) {
  if (n < 0 || (n > 0 && !problems)) return ORBX_ERR_ARG;
  if (n == 0) return ORBX_OK;
  size_t rows = 0;
  for (int i = 0; i < n; i++) {
    const orbx_status s = pose_check(problems[i]);
    if (s != ORBX_OK) return s;
    rows += (size_t)problems[i].n;
  }
  using orbx::pose::PoseDev;
  hipStream_t st = (hipStream_t)stream;
  // the records, then every problem's rows of scratch, then their active lists
  const size_t dev_bytes = sizeof(PoseDev) * n;
  const size_t scr_off = orbx::scratch_align(dev_bytes);
  const size_t act_off = scr_off + rows * orbx::pose::kRow * 8;
  return orbx::with_stream_block(act_off + rows * 4 + 16, st, [&](uint8_t* d) {
    std::vector<PoseDev> pd(n);
    size_t r = 0;
    for (int i = 0; i < n; i++) {
      pd[i].p = problems[i];
      pd[i].scratch = (double*)(d + scr_off) + r * orbx::pose::kRow;
      pd[i].act = (int*)(d + act_off) + r;
      r += (size_t)problems[i].n;
    }
    // pageable source: hipMemcpyAsync returns once pd is staged, so pd may go
    hipError_t e = hipMemcpyAsync(d, pd.data(), dev_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(orbx::pose::k_pose_optimization, dim3(n), dim3(orbx::pose::PBS), 0, st, (const PoseDev*)d);
      e = hipGetLastError();
    }
    return e;
  });
}

// optsim3.hip -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1220-1456), one block per problem, the
// whole schedule on the device: optimize(5), the pair-wise outlier pass on the stored errors, the
// early return, optimize(nMore), the final inlier count.
//
// The problem is one 7-DoF VertexSim3Expmap with two Huber edges per correspondence
// (EdgeSim3ProjectXYZ, EdgeInverseSim3ProjectXYZ).  Neither edge has an analytic Jacobian, so g2o
// differentiates numerically: per edge and linearisation, 14 error evaluations at the estimates
// Sim3(+-1e-9 e_d) * S.  Those 14 estimates (and the inverses the e21 edges map through) are the same
// for every edge, so 15 lanes compute them once into LDS by exactly the per-edge expression and each
// edge's thread then evaluates its 15 errors from there: the reference's push/oplus/pop arithmetic at
// 1/(2n) of its transcendental work.  The sums g2o forms in edge insertion order (activeRobustChi2,
// the 28 upper H entries, the 7 b entries) are taken in that order, one FP64 chain per entry on its
// own lane over LDS-staged per-edge terms, chunk by chunk (the result does not depend on the chunk
// size: a chain carries across chunks).  With exp_det / sincos_d for g2o::Sim3's exp and the shared
// Eigen-LDLT restatement at N = 7 and Levenberg step (orbx_lm.h; the literal's lm_trial /
// lm_iteration_end are its twin) the kernel reproduces tests/optsim3_literal.py bit for bit.
//
// Bound: latency (dependent FP64 chains of length 2n per LM iteration and trial; the serial 7x7
// solve and Sim3 exp on one lane); throughput comes from problems in flight.  Algorithmic bytes per
// linearisation: 36 B of input per edge, 16 B of stored error, 288 B of staged terms in LDS.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "orbx_device.h"
#include "orbx_scratch.h"
#include "orbx_internal.h"
#include "orbx_lm.h"
#include "orbx_sim3.h"
#include "../../include/orbx_debug.h"

namespace orbx {
namespace osim3 {

using namespace lm;
using namespace g2osim3;  // Sim3, sim3_exp / sim3_mul / sim3_inverse / oplus_unit (orbx_sim3.h)

constexpr int BS = 256;
constexpr int kCh = BS;              // edges staged per chunk (128 pairs), one thread each
constexpr int kTerm = 36, kTs = 37;  // 28 H (upper) | 7 b | chi term, at an odd row stride
constexpr int kChiCh = kCh * kTs;    // chi terms per trial pass (one double each)

struct Pair {  // an estimate and its inverse (what the e12 resp. e21 edges map through)
  Sim3 S, Si;
};

struct Dev {
  orbx_optimize_sim3_problem p;
  double* err;  // n x 4: the stored _error of e12 (x, y) and e21 (x, y) of each pair
  int* act;     // n: active pair ids in insertion order
};

struct Edge {
  double X[3], obs[2], info, fx, fy, cx, cy;
};

// edge k of the active list: pair act[k >> 1]; even = e12 (X2 through S into camera 1), odd = e21
__device__ __forceinline__ Edge load_edge(const orbx_optimize_sim3_problem& P, int i, int type) {
  Edge e;
  const float* X = type ? P.x3dc1 : P.x3dc2;
  const float* o = type ? P.obs2 : P.obs1;
  const float* K = type ? P.K2 : P.K1;
#pragma unroll
  for (int k = 0; k < 3; k++) e.X[k] = X[3 * i + k];
  e.obs[0] = o[2 * i];
  e.obs[1] = o[2 * i + 1];
  e.info = type ? P.inv_sigma2_2[i] : P.inv_sigma2_1[i];
  e.fx = K[0]; e.fy = K[1]; e.cx = K[2]; e.cy = K[3];
  return e;
}
// computeError of either edge through T (the estimate for e12, its inverse for e21):
// obs - cam_map(project(T.map(X)))
__device__ __forceinline__ void edge_error(const Sim3& T, const Edge& e, double& e0, double& e1) {
  double r[3];
  qrot(T.q, e.X, r);
  const double p0 = T.s * r[0] + T.t[0], p1 = T.s * r[1] + T.t[1], p2 = T.s * r[2] + T.t[2];
  e0 = e.obs[0] - (p0 / p2 * e.fx + e.cx);
  e1 = e.obs[1] - (p1 / p2 * e.fy + e.cy);
}
__device__ __forceinline__ double chi2_of(double info, double e0, double e1) {
  double s = e0 * (info * e0);
  s += e1 * (info * e1);
  return s;
}
// RobustKernelHuber::robustify (dsqr is a float member)
__device__ __forceinline__ void huber(double delta, float dsqr, double chi, double& rho0, double& rho1) {
  if (chi <= dsqr) {
    rho0 = chi;
    rho1 = 1.;
  } else {
    const double sq = __builtin_sqrt(chi);
    rho0 = 2 * sq * delta - dsqr;
    rho1 = delta / sq;
  }
}

struct Shared {
  Sim3 S, bak;
  Pair pert[15];  // [0] the estimate; [1 + 2d], [2 + 2d]: oplus(+delta e_d), oplus(-delta e_d)
  Pair trial;
  double H[49], b[7], x[7];
  Step lm;  // lambda, ni, currentChi, iniChi, rho, qmax, nBad (orbx_lm.h)
  int ok2, go, term, trials;
  int scan[BS / 64];
};

__device__ __forceinline__ const Sim3& side(const Pair& p, int type) { return type ? p.Si : p.S; }

__global__ __launch_bounds__(BS) void k_optimize_sim3(const Dev* __restrict__ probs) {
  __shared__ Shared S;
  __shared__ double sterm[kCh * kTs];
  const Dev& D = probs[blockIdx.x];
  const orbx_optimize_sim3_problem& P = D.p;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n = P.n_dev ? min(max(*P.n_dev, 0), P.n) : P.n;  // device-sized: P.n is the capacity
  double* err = D.err;
  int* act = D.act;
  const bool fix_scale = P.fix_scale != 0;
  const double delta = (double)__builtin_sqrtf(P.th2);  // const float deltaHuber = sqrt(th2)
  const float dsqr = (float)(delta * delta);
  const double th2 = (double)P.th2;

  for (int i = tid; i < n; i += BS) {
    P.inlier[i] = 1;
    act[i] = i;
  }
  if (tid < 8) P.S12_out[tid] = P.S12[tid];
  if (tid == 0) {
    S.S.q.x = P.S12[0]; S.S.q.y = P.S12[1]; S.S.q.z = P.S12[2]; S.S.q.w = P.S12[3];
    S.S.t[0] = P.S12[4]; S.S.t[1] = P.S12[5]; S.S.t[2] = P.S12[6];
    S.S.s = P.S12[7];
    S.trials = 0;
  }
  __threadfence_block();
  __syncthreads();
  int nact = n, nBad = 0, nIn = 0, its0 = 0, its1 = 0;
  bool early = false;
  for (int phase = 0; phase < 2; phase++) {
    const int max_its = phase == 0 ? 5 : (nBad > 0 ? 10 : 5);
    const int nedge = 2 * nact;
    int its = 0;
    if (nact > 0) {
      for (int iter = 0; iter < max_its; iter++) {
        its++;
        // the estimate and its 14 perturbations, each with its inverse: one lane each
        if (tid < 15) {
          const int d = tid == 0 ? -1 : (tid - 1) >> 1;
          const double step = (tid & 1) ? 1e-9 : -1e-9;
          Pair pr;
          pr.S = tid == 0 ? S.S : oplus_unit(S.S, d, step, fix_scale);
          pr.Si = sim3_inverse(pr.S);
          S.pert[tid] = pr;
        }
        __syncthreads();
        // computeActiveErrors + activeRobustChi2 (currentChi) and buildSystem's terms (numeric
        // linearizeOplus + constructQuadraticForm), a chunk of kCh active edges at a time into LDS,
        // each entry summed in insertion order by its own lane
        double acc = 0.0;  // wave 0, lanes 0..35: H upper (0..27), b (28..34), chi (35)
        for (int c0 = 0; c0 < nedge; c0 += kCh) {
          const int k = c0 + tid;
          if (k < nedge) {
            const int i = act[k >> 1], type = k & 1;
            const Edge e = load_edge(P, i, type);
            double e0, e1;
            edge_error(side(S.pert[0], type), e, e0, e1);
            err[4 * i + 2 * type] = e0;
            err[4 * i + 2 * type + 1] = e1;
            double* tr = sterm + tid * kTs;
            const double chi = chi2_of(e.info, e0, e1);
            double rho0, rho1;
            huber(delta, dsqr, chi, rho0, rho1);
            tr[35] = rho0;
            const double scalar = 1.0 / (2 * 1e-9);
            double J0[7], J1[7];
#pragma unroll
            for (int d = 0; d < 7; d++) {
              double p0, p1, m0, m1;
              edge_error(side(S.pert[1 + 2 * d], type), e, p0, p1);
              edge_error(side(S.pert[2 + 2 * d], type), e, m0, m1);
              J0[d] = scalar * (p0 - m0);
              J1[d] = scalar * (p1 - m1);
            }
            const double w = rho1 * e.info;  // robustInformation
            const double om0 = (-(e.info * e0)) * rho1, om1 = (-(e.info * e1)) * rho1;
            int q = 0;
#pragma unroll
            for (int r = 0; r < 7; r++)
#pragma unroll
              for (int cc = r; cc < 7; cc++) tr[q++] = (J0[r] * w) * J0[cc] + (J1[r] * w) * J1[cc];
#pragma unroll
            for (int r = 0; r < 7; r++) tr[28 + r] = J0[r] * om0 + J1[r] * om1;
          }
          __syncthreads();
          if (wid == 0 && lane < kTerm) acc = lds_chain(sterm + lane, min(kCh, nedge - c0), kTs, acc, false);
          __syncthreads();
        }
        if (wid == 0 && lane < kTerm) {
          if (lane < 28) {
            int r, c;
            tri_rc<7>(lane, r, c);
            S.H[7 * r + c] = acc;
            S.H[7 * c + r] = acc;
          } else if (lane < 35) {
            S.b[lane - 28] = acc;
          } else {
            S.lm.currentChi = acc;
            S.lm.iniChi = acc;
          }
        }
        __syncthreads();
        if (tid == 0) {
          if (iter == 0) start(S.lm, lambda_init<7>(S.H));
          S.lm.qmax = 0;
        }
        __syncthreads();
        // ---- trials ----
        for (;;) {
          if (tid == 0) {
            S.bak = S.S;
            double Hd[49];  // registers: every index static
#pragma unroll
            for (int j = 0; j < 49; j++) Hd[j] = S.H[j];
#pragma unroll
            for (int j = 0; j < 7; j++) Hd[8 * j] += S.lm.lambda;
            double x[7];
            const bool ok2 = ldlt<7>(Hd, S.b, x);
            S.ok2 = ok2;
            S.trials++;
            if (ok2) {
              if (fix_scale) x[6] = 0;  // oplusImpl zeroes the solver's x in place
              S.S = sim3_mul(sim3_exp(x), S.S);
            }
#pragma unroll
            for (int j = 0; j < 7; j++) S.x[j] = ok2 ? x[j] : 0.0;
            S.trial.S = S.S;
            S.trial.Si = sim3_inverse(S.S);
          }
          __syncthreads();
          double tempChi = 0.0;  // thread 0: activeRobustChi2 at the trial estimate, insertion order
          for (int c0 = 0; c0 < nedge; c0 += kChiCh) {
            for (int k = c0 + tid; k < min(nedge, c0 + kChiCh); k += BS) {
              const int i = act[k >> 1], type = k & 1;
              const Edge e = load_edge(P, i, type);
              double e0, e1;
              edge_error(side(S.trial, type), e, e0, e1);
              err[4 * i + 2 * type] = e0;
              err[4 * i + 2 * type + 1] = e1;
              double rho0, rho1;
              huber(delta, dsqr, chi2_of(e.info, e0, e1), rho0, rho1);
              sterm[k - c0] = rho0;
            }
            __syncthreads();
            if (tid == 0) tempChi = lds_chain(sterm, min(kChiCh, nedge - c0), 1, tempChi, false);
            __syncthreads();
          }
          if (tid == 0) {
            const bool ok2 = S.ok2;
            double scale = 0.0;
            if (ok2)
              for (int j = 0; j < 7; j++) scale += S.x[j] * (S.lm.lambda * S.x[j] + S.b[j]);
            const Verdict v = trial<Cube::kProduct>(S.lm, tempChi, scale, ok2);
            if (!v.accept) S.S = S.bak;  // pop; the rejected trial's errors stay in the edges
            S.go = v.go;
          }
          __syncthreads();
          if (!S.go) break;
        }
        if (tid == 0) S.term = iteration_end(S.lm);
        __syncthreads();
        if (S.term) break;
      }
    }
    if (phase == 0) its0 = its; else its1 = its;
    // ---- the pair test on the STORED errors (:1393-1412, :1433-1448); after optimize(5) an ordered
    // block scan compacts the survivors in place (a write lands at or below the slot it was read from)
    __threadfence_block();
    __syncthreads();
    int base = 0;
    for (int c0 = 0; c0 < nact; c0 += BS) {
      const int k = c0 + tid;
      int i = -1, keep = 0;
      if (k < nact) {
        i = act[k];
        const double c12 = chi2_of((double)P.inv_sigma2_1[i], err[4 * i], err[4 * i + 1]);
        const double c21 = chi2_of((double)P.inv_sigma2_2[i], err[4 * i + 2], err[4 * i + 3]);
        keep = !(c12 > th2 || c21 > th2);
        if (!keep) P.inlier[i] = 0;
      }
      compact_chunk<BS>(keep, S.scan, base, [&](int slot) {
        if (phase == 0) act[slot] = i;  // (the second pass only counts)
      });
    }
    __threadfence_block();
    __syncthreads();
    if (phase == 0) {
      nBad = nact - base;
      nact = base;
      if (n - nBad < 10) {  // return 0: g2oS12 is not written back, the nulled matches stay nulled
        early = true;
        break;
      }
    } else {
      nIn = base;
    }
  }
  if (tid == 0) {
    if (!early) {
      P.S12_out[0] = S.S.q.x; P.S12_out[1] = S.S.q.y; P.S12_out[2] = S.S.q.z; P.S12_out[3] = S.S.q.w;
      P.S12_out[4] = S.S.t[0]; P.S12_out[5] = S.S.t[1]; P.S12_out[6] = S.S.t[2];
      P.S12_out[7] = S.S.s;
    }
    *P.n_in = early ? 0 : nIn;
    if (P.n_bad) *P.n_bad = nBad;
    if (P.iterations) {
      P.iterations[0] = its0;
      P.iterations[1] = its1;
    }
    if (P.trials) *P.trials = S.trials;
  }
}

__global__ void k_debug_exp(const double* __restrict__ x, int n, double* __restrict__ y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = exp_det(x[i]);
}

__global__ void k_debug_sim3_exp(const double* __restrict__ in, int fix_scale, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double u[7];
#pragma unroll
  for (int k = 0; k < 7; k++) u[k] = in[k];
  if (fix_scale) u[6] = 0;
  Sim3 S;
  S.q.x = in[7]; S.q.y = in[8]; S.q.z = in[9]; S.q.w = in[10];
  S.t[0] = in[11]; S.t[1] = in[12]; S.t[2] = in[13];
  S.s = in[14];
  const Sim3 r = sim3_mul(sim3_exp(u), S);
  out[0] = r.q.x; out[1] = r.q.y; out[2] = r.q.z; out[3] = r.q.w;
  out[4] = r.t[0]; out[5] = r.t[1]; out[6] = r.t[2];
  out[7] = r.s;
}

}  // namespace osim3
}  // namespace orbx

// ------------------------------------------------------------------ C ABI
namespace {

orbx_status osim3_check(const orbx_optimize_sim3_problem& p) {
  if (p.n < 0) return ORBX_ERR_ARG;
  if (!p.S12_out || !p.n_in) return ORBX_ERR_ARG;
  if (p.n > 0 && (!p.x3dc1 || !p.x3dc2 || !p.obs1 || !p.obs2 || !p.inv_sigma2_1 || !p.inv_sigma2_2 || !p.inlier))
    return ORBX_ERR_ARG;
  return ORBX_OK;
}

}  // namespace

extern "C" orbx_status orbx_optimize_sim3(const orbx_optimize_sim3_problem* p, int device) {
  if (!p) return ORBX_ERR_ARG;
  const orbx_status chk = osim3_check(*p);
  if (chk != ORBX_OK) return chk;
  if (p->n_dev) return ORBX_ERR_ARG;  // device batches only
  const orbx_status dv = orbx::select_device(device);
  if (dv != ORBX_OK) return dv;
  using orbx::Staging;
  using orbx::osim3::Dev;
  const size_t n = (size_t)p->n;
  Staging S(device);  // pooled lease: no per-call allocation (orbx_scratch.h)
  const auto s_x1 = S.in(p->x3dc1, n * 3), s_x2 = S.in(p->x3dc2, n * 3);
  const auto s_o1 = S.in(p->obs1, n * 2), s_o2 = S.in(p->obs2, n * 2);
  const auto s_w1 = S.in(p->inv_sigma2_1, n), s_w2 = S.in(p->inv_sigma2_2, n);
  const auto s_dev = S.record<Dev>();
  const auto s_S = S.out<double>(8);
  const auto s_in = S.out<uint8_t>(n);
  const auto s_cnt = S.out<int32_t>(8);  // n_in | n_bad | iterations[2] | trials
  const auto s_err = S.device_only<double>(n * 4);
  const auto s_act = S.device_only<int>(n);
  const orbx_status cs = S.commit();
  if (cs != ORBX_OK) return cs;
  Dev pd;
  pd.p = *p;
  pd.p.x3dc1 = S.dev(s_x1);
  pd.p.x3dc2 = S.dev(s_x2);
  pd.p.obs1 = S.dev(s_o1);
  pd.p.obs2 = S.dev(s_o2);
  pd.p.inv_sigma2_1 = S.dev(s_w1);
  pd.p.inv_sigma2_2 = S.dev(s_w2);
  pd.p.S12_out = S.dev(s_S);
  pd.p.inlier = S.dev(s_in);
  int32_t* cnt = S.dev(s_cnt);
  pd.p.n_in = cnt;
  pd.p.n_bad = cnt + 1;
  pd.p.iterations = cnt + 2;
  pd.p.trials = cnt + 4;
  pd.err = S.dev(s_err);
  pd.act = S.dev(s_act);
  S.fill(s_dev, pd);
  hipError_t e = S.upload(Staging::Outputs::zeroed);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(orbx::osim3::k_optimize_sim3, dim3(1), dim3(orbx::osim3::BS), 0, S.stream(),
                       (const Dev*)S.dev(s_dev));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = S.download();
  if (e == hipSuccess) e = S.sync();
  if (e != hipSuccess) return ORBX_ERR_HIP;
  S.fetch(s_S, p->S12_out, 8);
  S.fetch(s_in, p->inlier, n);
  const int32_t* hc = S.host(s_cnt);
  *p->n_in = hc[0];
  if (p->n_bad) *p->n_bad = hc[1];
  if (p->iterations) std::memcpy(p->iterations, hc + 2, 8);
  if (p->trials) *p->trials = hc[4];
  return ORBX_OK;
}

extern "C" orbx_status orbx_optimize_sim3_device(const orbx_optimize_sim3_problem* problems, int n, void* stream) {
  if (n < 0 || (n > 0 && !problems)) return ORBX_ERR_ARG;
  if (n == 0) return ORBX_OK;
  using orbx::osim3::Dev;
  size_t rows = 0;
  for (int i = 0; i < n; i++) {
    const orbx_status s = osim3_check(problems[i]);
    if (s != ORBX_OK) return s;
    rows += (size_t)problems[i].n;
  }
  hipStream_t st = (hipStream_t)stream;
  // the records, then every problem's rows of errors, then their active lists
  const size_t dev_bytes = sizeof(Dev) * n;
  const size_t err_off = orbx::scratch_align(dev_bytes);
  const size_t act_off = err_off + rows * 32;
  return orbx::with_stream_block(act_off + rows * 4 + 16, st, [&](uint8_t* d) {
    std::vector<Dev> pd(n);
    size_t r = 0;
    for (int i = 0; i < n; i++) {
      pd[i].p = problems[i];
      pd[i].err = (double*)(d + err_off) + r * 4;
      pd[i].act = (int*)(d + act_off) + r;
      r += (size_t)problems[i].n;
    }
    // pageable source: hipMemcpyAsync returns once pd is staged, so pd may go
    hipError_t e = hipMemcpyAsync(d, pd.data(), dev_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(orbx::osim3::k_optimize_sim3, dim3(n), dim3(orbx::osim3::BS), 0, st, (const Dev*)d);
      e = hipGetLastError();
    }
    return e;
  });
}

// ------------------------------------------------------------------ debug probes (orbx_debug.h)
extern "C" int orbx_debug_lm_step(double state[5], int counts[2], double tempChi, double scale, int ok2,
                                  int cube_kind, int ops) {  // the host build of orbx_lm.h's step
  if (!state || !counts || cube_kind < 0 || cube_kind > 1 || ops < 1 || ops > 3) return ORBX_ERR_ARG;
  namespace lm = orbx::lm;
  lm::Step s = {state[0], state[1], state[2], state[3], state[4], counts[0], counts[1]};
  int r = 0;
  if (ops & 1) {
    const lm::Verdict v = cube_kind ? lm::trial<lm::Cube::kRounded>(s, tempChi, scale, ok2 != 0)
                                    : lm::trial<lm::Cube::kProduct>(s, tempChi, scale, ok2 != 0);
    r |= (v.accept ? 1 : 0) | (v.go ? 2 : 0);
  }
  if ((ops & 2) && lm::iteration_end(s)) r |= 4;
  state[0] = s.lambda; state[1] = s.ni; state[2] = s.currentChi; state[3] = s.iniChi; state[4] = s.rho;
  counts[0] = s.qmax;
  counts[1] = s.nBad;
  return r;
}

extern "C" int orbx_debug_exp(const double* x, int n, double* y, int device) {
  if (n < 0 || (n > 0 && (!x || !y))) return ORBX_ERR_ARG;
  const orbx_status dv = orbx::select_device(device);
  if (dv != ORBX_OK) return dv;
  if (n == 0) return ORBX_OK;
  orbx::Staging S(device);
  const auto s_x = S.in(x, (size_t)n);
  const auto s_y = S.out<double>((size_t)n);
  const orbx_status cs = S.commit();
  if (cs != ORBX_OK) return cs;
  hipError_t e = S.upload(orbx::Staging::Outputs::skipped);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(orbx::osim3::k_debug_exp, dim3((n + 255) / 256), dim3(256), 0, S.stream(),
                       (const double*)S.dev(s_x), n, S.dev(s_y));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = S.download();
  if (e == hipSuccess) e = S.sync();
  if (e != hipSuccess) return ORBX_ERR_HIP;
  S.fetch(s_y, y, (size_t)n);
  return ORBX_OK;
}

extern "C" int orbx_debug_sim3_exp(const double update[7], const double S[8], int fix_scale, double out[8],
                                   int device) {
  if (!update || !S || !out) return ORBX_ERR_ARG;
  const orbx_status dv = orbx::select_device(device);
  if (dv != ORBX_OK) return dv;
  double in[15];  // update | S, as the kernel reads them
  std::memcpy(in, update, 56);
  std::memcpy(in + 7, S, 64);
  orbx::Staging G(device);
  const auto s_in = G.in(in, 15);
  const auto s_out = G.out<double>(8);
  const orbx_status cs = G.commit();
  if (cs != ORBX_OK) return cs;
  hipError_t e = G.upload(orbx::Staging::Outputs::skipped);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(orbx::osim3::k_debug_sim3_exp, dim3(1), dim3(64), 0, G.stream(), (const double*)G.dev(s_in),
                       fix_scale, G.dev(s_out));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = G.download();
  if (e == hipSuccess) e = G.sync();
  if (e != hipSuccess) return ORBX_ERR_HIP;
  G.fetch(s_out, out, 8);
  return ORBX_OK;
}

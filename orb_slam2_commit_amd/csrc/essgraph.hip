// essgraph.hip -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:888-1218), the pose graph of
// LoopClosing::CorrectLoop: one Sim3 vertex per keyframe (the loop keyframe fixed), EdgeSim3 edges
// with identity information, g2o's numeric Jacobians, Levenberg from lambda = 1e-16, optimize(20), then
// the SE3 recovery of the keyframes and the double-Sim3 correction of the map points.
//
// k_eg_measure   one thread per edge: the measurement Sji = Sjw * Swi from the pose table its kind
//                selects; the estimates start at Scw.
// k_eg_lm        ONE workgroup runs the whole Levenberg loop, no host round trip per trial:
//   linearise    one edge per wave: lane 0 the error (C * v0 * v1^-1).log(), lanes 1..28 the 28
//                perturbed errors of BaseBinaryEdge::linearizeOplus (oplus(+-1e-9 e_d) on either vertex),
//                then the edge's J0^T J0, J0^T J1, J1^T J1, J0^T (-e), J1^T (-e) and chi2 across the lanes.
//   assemble     one thread per Hessian entry: a vertex's diagonal block and b segment summed over its
//                incident edges, an off-diagonal block over the edges joining that pair, both in edge
//                order through CSR lists made on the host (no atomics, a fixed order); chi2 is one
//                sequential chain over the edges.
//   solve        H is a block envelope: block row r holds block columns first[r]..r, a scalar row
//                contiguous, in HBM.  LDL^T without pivoting, every entry updated for k ascending by
//                a_ij <- a_ij - (l_ik d_k) l_jk: per block column, the updates from earlier block
//                columns run one thread per entry, one thread factors the 7x7 diagonal block, one thread
//                per row below finishes its seven entries.  Forward substitution, the division by D and
//                back substitution run on wave 0 (seven rows of a block row across lanes).  Entries
//                outside the envelope are structural zeros and are skipped.  No MFMA: its fused
//                accumulation would change the rounding.
//   control      optimization_algorithm_levenberg.cpp as oracle/poseopt.cpp restates it (orbx_lm.h's
//                Step, shared with the other Levenberg kernels), at 7 (n - 1) unknowns, with the user's
//                lambda_init.
// k_eg_finish    one thread per vertex (Scw_out, Tiw) and per map point (the correction).
//
// Everything is FP64 from basic IEEE operations (log_det / acos_det / exp_det / sincos_d), so the
// kernels reproduce tests/essgraph_literal.py bit for bit.
//
// Bound: latency.  The factorisation runs three workgroup barriers per block column on one CU and the
// substitutions on one wave; linearisation (29 Sim3 logs per edge) spreads over the workgroup's waves
// only.  Bytes per trial: the envelope is read and written once (49 * 8 B per block), plus 1,296 B of
// per-edge terms per linearisation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "orbx_device.h"
#include "orbx_scratch.h"
#include "orbx_internal.h"
#include "orbx_lm.h"
#include "orbx_sim3.h"
#include "../../include/orbx_debug.h"

namespace orbx {
namespace essgraph {

using namespace lm;
using namespace g2osim3;

constexpr int BS = 512, NW = BS / 64;
constexpr int kT = 162;  // per-edge terms: J0^T J0 (49) | J0^T J1 (49) | J1^T J1 (49) | b0 (7) | b1 (7) | chi2

struct Dev {
  int n, nf, E, N, npairs, fix_scale, iterations, npts;
  double lambda_init;
  // the problem (device)
  const double* Scw;
  const double* Snc;
  const float* Xw;
  const int32_t* pref;
  // structure (device copies of the host plan)
  const int32_t* ev0;
  const int32_t* ev1;
  const int32_t* ekind;
  const int32_t* hidx;   // n: Hessian index of a vertex, -1 = fixed
  const int32_t* hv;     // nf: vertex of a Hessian index
  const int32_t* vptr;   // n + 1, into vinc
  const int32_t* vinc;   // incident edges of a vertex in edge order: 2 * edge + side
  const int32_t* prow;   // npairs: block row (the larger Hessian index) and column of an off-diagonal block
  const int32_t* pcol;
  const int32_t* pptr;   // npairs + 1, into pinc
  const int32_t* pinc;   // the pair's edges in edge order: 2 * edge + (vertex 0 is the ROW vertex)
  const int32_t* first;  // nf: first block column of a block row
  const int32_t* boff;   // nf + 1: block offset of a block row in the envelope
  const int32_t* cptr;   // nf + 1, into crow
  const int32_t* crow;   // block rows r > c whose envelope reaches block column c, ascending
  // work (device)
  double* meas;   // E x 8
  double* est;    // n x 8
  double* bak;    // n x 8
  double* T;      // E x kT
  double* Henv;   // the envelope of H
  double* Lenv;   // H + lambda I, then L (unit lower, strictly below the diagonal)
  double* dd;     // N: D
  double* b;      // N
  double* x;      // N
  double* y;      // N
  double* chain;  // max(E, N): terms of a sequential sum
  double* stats;  // iterations, trials, chi2_initial, chi2_final, solver_failures, ticks of linearise / solve /
                  // update (the rest of a trial) | probe: ok
  double* dbg_err;  // probes only: E x 7, E x 49, E x 49
  double* dbg_J0;
  double* dbg_J1;
  // outputs (device)
  double* Scw_out;
  float* Tcw_out;
  float* Xw_out;
  int32_t* o_iterations;
  int32_t* o_trials;
  double* o_chi0;
  double* o_chi1;
  int32_t* o_fail;
};

// scalar row i of the envelope: a(i, j) = base[env_row(D, i, c0) + j - c0], c0 its first stored column
__device__ __forceinline__ size_t env_row(const Dev& D, int i, int& c0) {
  const int r = i / 7, il = i - 7 * r, f = D.first[r];
  c0 = 7 * f;
  return 49 * (size_t)D.boff[r] + (size_t)il * (7 * (r - f + 1));
}

// EdgeSim3::computeError: (C * v0 * v1.inverse()).log()
__device__ __forceinline__ void edge_error(const Sim3& C, const Sim3& v0, const Sim3& v1, double (&e)[7]) {
  sim3_log(sim3_mul(sim3_mul(C, v0), sim3_inverse(v1)), e);
}

__global__ __launch_bounds__(256) void k_eg_measure(const Dev D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < D.E) {
    const double* tab = D.ekind[i] ? D.Snc : D.Scw;
    const Sim3 Swi = sim3_inverse(sim3_load(tab + 8 * D.ev0[i]));
    sim3_store(sim3_mul(sim3_load(tab + 8 * D.ev1[i]), Swi), D.meas + 8 * (size_t)i);
  }
  if (i < D.n) {
#pragma unroll
    for (int k = 0; k < 8; k++) D.est[8 * i + k] = D.Scw[8 * i + k];
  }
}

struct Shared {
  double E[NW][29 * 7];  // per wave: the error and its 28 perturbations
  double J[NW][98];      // per wave: J0 | J1, [k][d] (k the error entry)
  double Ld[49], d[7];   // the factored diagonal block of the current block column
  Step lm;  // lambda, ni, currentChi, iniChi, rho, qmax, nBad (orbx_lm.h)
  double chi0;
  int accept, go, term, trials, fails, fail, its;
  long long t_lin, t_solve, t_update;  // phase times in wall_clock64 ticks (thread 0)
};

// linearizeOplus + constructQuadraticForm's per-edge terms of every edge, one edge per wave
__device__ void eg_linearize(const Dev& D, Shared& S) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool fix_scale = D.fix_scale != 0;
  for (int e0 = 0; e0 < D.E; e0 += NW) {
    const int e = e0 + wid;
    const bool on = e < D.E;
    int v0 = 0, v1 = 0;
    bool f0 = true, f1 = true;
    if (on) {
      v0 = D.ev0[e];
      v1 = D.ev1[e];
      f0 = D.hidx[v0] < 0;
      f1 = D.hidx[v1] < 0;
    }
    if (on && lane < 29) {
      const int p = lane - 1, side = p >= 14, d = (p - 14 * side) >> 1;
      const double step = (p & 1) ? -1e-9 : 1e-9;
      const bool skip = lane > 0 && (side ? f1 : f0);  // a fixed vertex gets no Jacobian
      if (!skip) {
        Sim3 a = sim3_load(D.est + 8 * v0), b = sim3_load(D.est + 8 * v1);
        if (lane > 0) {
          if (side) b = oplus_unit(b, d, step, fix_scale);
          else a = oplus_unit(a, d, step, fix_scale);
        }
        double er[7];
        edge_error(sim3_load(D.meas + 8 * (size_t)e), a, b, er);
#pragma unroll
        for (int k = 0; k < 7; k++) S.E[wid][7 * lane + k] = er[k];
      }
    }
    __syncthreads();
    if (on) {
      const double scalar = 1.0 / (2 * 1e-9);
      for (int q = lane; q < 98; q += 64) {
        const int side = q >= 49, kd = q - 49 * side, k = kd / 7, d = kd - 7 * k;
        const bool fx = side ? f1 : f0;
        const double* Ep = S.E[wid] + 7 * (1 + 14 * side + 2 * d);
        const double v = fx ? 0.0 : scalar * (Ep[k] - Ep[7 + k]);
        S.J[wid][q] = v;
        if (D.dbg_J0) (side ? D.dbg_J1 : D.dbg_J0)[49 * (size_t)e + kd] = v;
      }
      if (D.dbg_err && lane < 7) D.dbg_err[7 * (size_t)e + lane] = S.E[wid][lane];
    }
    __syncthreads();
    if (on) {
      const double* J0 = S.J[wid];
      const double* J1 = S.J[wid] + 49;
      const double* er = S.E[wid];
      double* T = D.T + (size_t)kT * e;
      if (lane < 49) {
        const int r = lane / 7, c = lane - 7 * r;
        double a = J0[r] * J0[c], m = J0[r] * J1[c], z = J1[r] * J1[c];
#pragma unroll
        for (int k = 1; k < 7; k++) {
          a = a + J0[7 * k + r] * J0[7 * k + c];
          m = m + J0[7 * k + r] * J1[7 * k + c];
          z = z + J1[7 * k + r] * J1[7 * k + c];
        }
        T[lane] = a;
        T[49 + lane] = m;
        T[98 + lane] = z;
      } else if (lane < 63) {
        const int side = lane >= 56, r = lane - 49 - 7 * side;
        const double* J = side ? J1 : J0;
        double s = J[r] * (-er[0]);
#pragma unroll
        for (int k = 1; k < 7; k++) s = s + J[7 * k + r] * (-er[k]);
        T[147 + 7 * side + r] = s;
      } else {
        double s = er[0] * er[0];
#pragma unroll
        for (int k = 1; k < 7; k++) s = s + er[k] * er[k];
        T[161] = s;
        D.chain[e] = s;
      }
    }
    __syncthreads();
  }
}

// H's envelope and b from the per-edge terms; blocks of the envelope that no edge joins stay zero
__device__ void eg_assemble(const Dev& D) {
  const int tid = threadIdx.x;
  const int ndiag = D.nf * 56;
  for (int w = tid; w < ndiag + D.npairs * 49; w += BS) {
    if (w < ndiag) {
      const int h = w / 56, q = w - 56 * h, v = D.hv[h];
      double acc = 0.0;
      for (int it = D.vptr[v]; it < D.vptr[v + 1]; it++) {
        const int ed = D.vinc[it] >> 1, side = D.vinc[it] & 1;
        const double* T = D.T + (size_t)kT * ed;
        acc += q < 49 ? T[(side ? 98 : 0) + q] : T[147 + 7 * side + (q - 49)];
      }
      if (q < 49) {
        int c0;
        const size_t o = env_row(D, 7 * h + q / 7, c0);
        D.Henv[o + (7 * h + q % 7) - c0] = acc;
      } else {
        D.b[7 * h + (q - 49)] = acc;
      }
    } else {
      const int p = (w - ndiag) / 49, q = (w - ndiag) - 49 * p, a = q / 7, bb = q - 7 * a;
      double acc = 0.0;
      for (int it = D.pptr[p]; it < D.pptr[p + 1]; it++) {
        const int ed = D.pinc[it] >> 1, v0row = D.pinc[it] & 1;
        const double* T = D.T + (size_t)kT * ed + 49;
        acc += v0row ? T[7 * a + bb] : T[7 * bb + a];
      }
      int c0;
      const size_t o = env_row(D, 7 * D.prow[p] + a, c0);
      D.Henv[o + (7 * D.pcol[p] + bb) - c0] = acc;
    }
  }
}

// Lenv = LDL^T of Henv + lambda I; S.fail is set on an exactly zero pivot.  All threads.
__device__ void eg_factor(const Dev& D, Shared& S, double lambda) {
  const int tid = threadIdx.x;
  const size_t total = 49 * (size_t)D.boff[D.nf];
  for (size_t q = tid; q < total; q += BS) D.Lenv[q] = D.Henv[q];
  if (tid == 0) S.fail = 0;
  __syncthreads();
  for (int i = tid; i < D.N; i += BS) {
    int c0;
    const size_t o = env_row(D, i, c0);
    D.Lenv[o + i - c0] += lambda;
  }
  __syncthreads();
  double* L = D.Lenv;
  for (int c = 0; c < D.nf; c++) {
    const int cp = D.cptr[c], cnt = D.cptr[c + 1] - cp, fc = D.first[c];
    // (A) the updates from the block columns before c, one thread per entry, k ascending
    if (fc < c || cnt > 0) {
      for (int w = tid; w < (cnt + 1) * 49; w += BS) {
        const int rb = w / 49, q = w - 49 * rb, il = q / 7, jl = q - 7 * il;
        const int r = rb == 0 ? c : D.crow[cp + rb - 1];
        if (r == c && jl > il) continue;
        int ci, cj;
        double* ri = L + env_row(D, 7 * r + il, ci);
        const double* rj = L + env_row(D, 7 * c + jl, cj);
        const int k0 = ci > cj ? ci : cj;
        double a = ri[7 * c + jl - ci];
        for (int k = k0; k < 7 * c; k++) a -= (ri[k - ci] * D.dd[k]) * rj[k - cj];
        ri[7 * c + jl - ci] = a;
      }
      __syncthreads();
    }
    // (B1) the diagonal block, one thread, right-looking: each entry still takes its updates k ascending
    if (tid == 0) {
      double m[49];
#pragma unroll
      for (int il = 0; il < 7; il++) {
        int ci;
        const double* ri = L + env_row(D, 7 * c + il, ci);
#pragma unroll
        for (int jl = 0; jl < 7; jl++) m[7 * il + jl] = jl <= il ? ri[7 * c + jl - ci] : 0.0;
      }
      bool fail = false;
#pragma unroll
      for (int k = 0; k < 7; k++) {
        const double dk = m[8 * k];
        if (dk == 0.0) fail = true;
#pragma unroll
        for (int i = k + 1; i < 7; i++) {
          const double l = m[7 * i + k] / dk;
          const double wv = l * dk;
          m[7 * i + k] = l;  // before the row's own diagonal entry reads it
#pragma unroll
          for (int j = k + 1; j <= i; j++) m[7 * i + j] -= wv * m[7 * j + k];
        }
      }
      if (fail) S.fail = 1;
#pragma unroll
      for (int il = 0; il < 7; il++) {
        int ci;
        double* ri = L + env_row(D, 7 * c + il, ci);
#pragma unroll
        for (int jl = 0; jl < il; jl++) ri[7 * c + jl - ci] = m[7 * il + jl];
        D.dd[7 * c + il] = m[8 * il];
        S.d[il] = m[8 * il];
      }
#pragma unroll
      for (int q = 0; q < 49; q++) S.Ld[q] = m[q];
    }
    __syncthreads();
    // (B2) the rows below: one thread finishes a row's seven entries
    if (cnt > 0) {
      for (int w = tid; w < cnt * 7; w += BS) {
        const int rb = w / 7, il = w - 7 * rb, r = D.crow[cp + rb];
        int ci;
        double* ri = L + env_row(D, 7 * r + il, ci) + (7 * c - ci);
        double a[7];
#pragma unroll
        for (int j = 0; j < 7; j++) a[j] = ri[j];
#pragma unroll
        for (int j = 0; j < 7; j++) {
#pragma unroll
          for (int k = 0; k < j; k++) a[j] -= (a[k] * S.d[k]) * S.Ld[7 * j + k];
          a[j] = a[j] / S.d[j];
        }
#pragma unroll
        for (int j = 0; j < 7; j++) ri[j] = a[j];
      }
    }
    __syncthreads();
  }
}

// L y = b (k ascending per entry), y / D, L^T x = y (k descending per entry) into D.x.  Wave 0 only.
__device__ void eg_substitute(const Dev& D) {
  const int lane = threadIdx.x & 63;
  const double* L = D.Lenv;
  double* y = D.y;
  for (int r = 0; r < D.nf; r++) {
    double s = 0.0;
    const double* ri = L;
    int ci = 0;
    if (lane < 7) {
      ri = L + env_row(D, 7 * r + lane, ci);
      s = D.b[7 * r + lane];
      for (int k = ci; k < 7 * r; k++) s -= ri[k - ci] * y[k];
    }
#pragma unroll
    for (int t = 0; t < 6; t++) {
      const double yt = __shfl(s, t, 64);
      if (lane < 7 && lane > t) s -= ri[7 * r + t - ci] * yt;
    }
    if (lane < 7) y[7 * r + lane] = s;
    __threadfence_block();
  }
  for (int i = lane; i < D.N; i += 64) y[i] = y[i] / D.dd[i];
  __threadfence_block();
  for (int r = D.nf - 1; r >= 0; r--) {
    const int c0 = 7 * D.first[r], W = 7 * (r - D.first[r] + 1);
    const double* blk = L + 49 * (size_t)D.boff[r];  // row 7r + t at blk + t * W, column j at [j - c0]
    double s = lane < 7 ? y[7 * r + lane] : 0.0;
#pragma unroll
    for (int t = 6; t >= 1; t--) {
      const double xt = __shfl(s, t, 64);
      if (lane < t) s -= blk[(size_t)t * W + (7 * r + lane - c0)] * xt;
    }
    if (lane < 7) D.x[7 * r + lane] = s;
    double xs[7];
#pragma unroll
    for (int t = 0; t < 7; t++) xs[t] = __shfl(s, t, 64);
    for (int i = c0 + lane; i < 7 * r; i += 64) {
      double v = y[i];
#pragma unroll
      for (int t = 6; t >= 0; t--) v -= blk[(size_t)t * W + (i - c0)] * xs[t];
      y[i] = v;
    }
    __threadfence_block();
  }
}

// computeActiveErrors + the per-edge chi2 at the current estimates, one thread per edge
__device__ void eg_errors(const Dev& D) {
  for (int e = threadIdx.x; e < D.E; e += BS) {
    double er[7];
    edge_error(sim3_load(D.meas + 8 * (size_t)e), sim3_load(D.est + 8 * D.ev0[e]), sim3_load(D.est + 8 * D.ev1[e]), er);
    double s = er[0] * er[0];
#pragma unroll
    for (int k = 1; k < 7; k++) s = s + er[k] * er[k];
    D.chain[e] = s;
  }
}

__global__ __launch_bounds__(BS) void k_eg_lm(const Dev D) {
  __shared__ Shared S;
  const int tid = threadIdx.x;
  if (tid == 0) {
    S.trials = 0;
    S.fails = 0;
    S.its = 0;
    S.lm.currentChi = 0.0;
    S.chi0 = 0.0;
    S.t_lin = S.t_solve = S.t_update = 0;
  }
  __syncthreads();
  for (int iter = 0; iter < D.iterations; iter++) {
    long long t0 = tid == 0 ? wall_clock64() : 0;
    eg_linearize(D, S);  // its lane 0 is computeActiveErrors at the current estimates
    __syncthreads();
    eg_assemble(D);
    if (tid == 0) {
      const double chi = lds_chain(D.chain, D.E, 1, 0.0, false);
      S.lm.currentChi = chi;
      S.lm.iniChi = chi;
      if (iter == 0) S.chi0 = chi;
      S.its++;
    }
    __syncthreads();
    if (tid == 0) S.t_lin += wall_clock64() - t0;
    if (tid == 0) {
      if (iter == 0) start(S.lm, D.lambda_init);  // setUserLambdaInit: computeLambdaInit returns the user's value
      S.lm.qmax = 0;
    }
    __syncthreads();
    for (;;) {
      const double lambda = S.lm.lambda;
      t0 = tid == 0 ? wall_clock64() : 0;
      for (int q = tid; q < 8 * D.n; q += BS) D.bak[q] = D.est[q];  // push
      eg_factor(D, S, lambda);
      const bool ok2 = !S.fail;
      if (ok2 && tid < 64) eg_substitute(D);
      __syncthreads();
      if (tid == 0) {
        const long long t1 = wall_clock64();
        S.t_solve += t1 - t0;
        t0 = t1;
      }
      if (ok2) {
        for (int h = tid; h < D.nf; h += BS) {
          double u[7];
#pragma unroll
          for (int k = 0; k < 7; k++) u[k] = D.x[7 * h + k];
          if (D.fix_scale) {  // oplusImpl zeroes the solver's x in place
            u[6] = 0;
            D.x[7 * h + 6] = 0;
          }
          const int v = D.hv[h];
          sim3_store(sim3_mul(sim3_exp(u), sim3_load(D.bak + 8 * v)), D.est + 8 * v);
        }
      }
      __syncthreads();
      eg_errors(D);
      __syncthreads();
      double tempChi = 0.0;
      if (tid == 0) tempChi = lds_chain(D.chain, D.E, 1, 0.0, false);
      __syncthreads();
      if (ok2)
        for (int j = tid; j < D.N; j += BS) D.chain[j] = D.x[j] * (lambda * D.x[j] + D.b[j]);
      __syncthreads();
      if (tid == 0) {
        S.trials++;
        if (!ok2) S.fails++;
        const double scale = ok2 ? lds_chain(D.chain, D.N, 1, 0.0, false) : 0.0;
        const Verdict v = trial<Cube::kProduct>(S.lm, tempChi, scale, ok2);
        S.accept = v.accept;  // else: pop
        S.go = v.go;
      }
      __syncthreads();
      if (!S.accept)
        for (int q = tid; q < 8 * D.n; q += BS) D.est[q] = D.bak[q];
      __syncthreads();
      if (tid == 0) S.t_update += wall_clock64() - t0;
      if (!S.go) break;
    }
    if (tid == 0) S.term = iteration_end(S.lm);
    __syncthreads();
    if (S.term) break;
  }
  if (tid == 0) {
    D.stats[0] = S.its;
    D.stats[1] = S.trials;
    D.stats[2] = S.chi0;
    D.stats[3] = S.lm.currentChi;
    D.stats[4] = S.fails;
    D.stats[5] = (double)S.t_lin;
    D.stats[6] = (double)S.t_solve;
    D.stats[7] = (double)S.t_update;
  }
}

__global__ __launch_bounds__(256) void k_eg_finish(const Dev D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < D.n) {
    const Sim3 S = sim3_load(D.est + 8 * i);
    sim3_store(S, D.Scw_out + 8 * i);
    double R[9];
    qmat(S.q, R);
    const double is = 1. / S.s;
    float* T = D.Tcw_out + 12 * i;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
      for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
      T[4 * r + 3] = (float)(S.t[r] * is);
    }
  }
  if (i < D.npts) {
    const int r = D.pref[i];
    float o[3] = {D.Xw[3 * i], D.Xw[3 * i + 1], D.Xw[3 * i + 2]};
    if (r >= 0 && r < D.n) {
      const double X[3] = {(double)o[0], (double)o[1], (double)o[2]};
      double a[3], c[3];
      sim3_map(sim3_load(D.Scw + 8 * r), X, a);
      sim3_map(sim3_inverse(sim3_load(D.est + 8 * r)), a, c);
#pragma unroll
      for (int k = 0; k < 3; k++) o[k] = (float)c[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) D.Xw_out[3 * i + k] = o[k];
  }
  if (i == 0) {
    if (D.o_iterations) *D.o_iterations = (int32_t)D.stats[0];
    if (D.o_trials) *D.o_trials = (int32_t)D.stats[1];
    if (D.o_chi0) *D.o_chi0 = D.stats[2];
    if (D.o_chi1) *D.o_chi1 = D.stats[3];
    if (D.o_fail) *D.o_fail = (int32_t)D.stats[4];
  }
}

// ---- probes
__global__ __launch_bounds__(BS) void k_eg_linearize(const Dev D) {
  __shared__ Shared S;
  eg_linearize(D, S);
  __syncthreads();
  eg_assemble(D);
}

__global__ __launch_bounds__(BS) void k_eg_solve(const Dev D, double lambda) {
  __shared__ Shared S;
  eg_factor(D, S, lambda);
  const bool ok = !S.fail;
  if (ok && threadIdx.x < 64) eg_substitute(D);
  if (threadIdx.x == 0) D.stats[0] = ok ? 1.0 : 0.0;
}

__global__ void k_debug_unary(const double* __restrict__ x, int n, double* __restrict__ y, int what) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = what ? acos_det(x[i]) : log_det(x[i]);
}

__global__ void k_debug_sim3_log(const double* __restrict__ S, int n, double* __restrict__ out,
                                 int32_t* __restrict__ branch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r[7];
  int br;
  sim3_log(sim3_load(S + 8 * (size_t)i), r, &br);
#pragma unroll
  for (int k = 0; k < 7; k++) out[7 * (size_t)i + k] = r[k];
  branch[i] = br;
}

// ------------------------------------------------------------------ the host's plan
struct Plan {
  int n = 0, nf = 0, E = 0, N = 0, npairs = 0;
  size_t nblk = 0;
  std::vector<int32_t> ints;  // every structure array back to back; offsets in elements
  size_t o_ev0, o_ev1, o_kind, o_hidx, o_hv, o_vptr, o_vinc, o_prow, o_pcol, o_pptr, o_pinc, o_first, o_boff, o_cptr,
      o_crow;
  std::vector<int32_t> first, boff;  // host copies (dense <-> envelope)
};

orbx_status check(const orbx_essential_graph_problem& p, bool host_points) {
  if (p.n_vertices < 2 || p.n_edges < 0 || p.n_points < 0 || p.iterations < 0 || !(p.lambda_init > 0))
    return ORBX_ERR_ARG;
  if (!p.vertex_id || !p.Scw || !p.Snc) return ORBX_ERR_ARG;
  if (p.fixed_vertex < 0 || p.fixed_vertex >= p.n_vertices) return ORBX_ERR_ARG;
  if (p.n_edges > 0 && (!p.edge_v0 || !p.edge_v1 || !p.edge_kind)) return ORBX_ERR_ARG;
  if (p.n_points > 0 && (!p.Xw || !p.point_ref)) return ORBX_ERR_ARG;
  if ((long long)7 * (p.n_vertices - 1) > 0x7fffffffLL / 8) return ORBX_ERR_ARG;
  for (int i = 1; i < p.n_vertices; i++)
    if (p.vertex_id[i] <= p.vertex_id[i - 1]) return ORBX_ERR_ARG;
  for (int e = 0; e < p.n_edges; e++) {
    const int a = p.edge_v0[e], b = p.edge_v1[e];
    if (a < 0 || a >= p.n_vertices || b < 0 || b >= p.n_vertices || a == b || p.edge_kind[e] > 1) return ORBX_ERR_ARG;
  }
  if (host_points)
    for (int i = 0; i < p.n_points; i++)
      if (p.point_ref[i] < 0 || p.point_ref[i] >= p.n_vertices) return ORBX_ERR_ARG;
  return ORBX_OK;
}

bool make_plan(const orbx_essential_graph_problem& p, Plan& P) {
  const int n = p.n_vertices, E = p.n_edges, nf = n - 1;
  P.n = n; P.nf = nf; P.E = E; P.N = 7 * nf;
  std::vector<int32_t> hidx(n), hv(nf);
  for (int v = 0, h = 0; v < n; v++) {
    hidx[v] = v == p.fixed_vertex ? -1 : h;
    if (v != p.fixed_vertex) hv[h++] = v;
  }
  std::vector<int32_t> vptr(n + 1, 0), vinc;
  for (int e = 0; e < E; e++) {
    vptr[p.edge_v0[e] + 1]++;
    vptr[p.edge_v1[e] + 1]++;
  }
  for (int v = 0; v < n; v++) vptr[v + 1] += vptr[v];
  vinc.resize(vptr[n]);
  {
    std::vector<int32_t> fill(vptr.begin(), vptr.end() - 1);
    for (int e = 0; e < E; e++) {
      vinc[fill[p.edge_v0[e]]++] = 2 * e;
      vinc[fill[p.edge_v1[e]]++] = 2 * e + 1;
    }
  }
  std::map<std::pair<int, int>, std::vector<int32_t>> pairs;  // (row, column) -> 2 * edge + (v0 is the row)
  for (int e = 0; e < E; e++) {
    const int h0 = hidx[p.edge_v0[e]], h1 = hidx[p.edge_v1[e]];
    if (h0 < 0 || h1 < 0) continue;
    const bool v0row = h0 > h1;
    pairs[std::make_pair(v0row ? h0 : h1, v0row ? h1 : h0)].push_back(2 * e + (v0row ? 1 : 0));
  }
  P.npairs = (int)pairs.size();
  std::vector<int32_t> prow, pcol, pptr(1, 0), pinc;
  P.first.resize(nf);
  for (int r = 0; r < nf; r++) P.first[r] = r;
  for (const auto& kv : pairs) {
    prow.push_back(kv.first.first);
    pcol.push_back(kv.first.second);
    pinc.insert(pinc.end(), kv.second.begin(), kv.second.end());
    pptr.push_back((int32_t)pinc.size());
    P.first[kv.first.first] = std::min(P.first[kv.first.first], (int32_t)kv.first.second);
  }
  P.boff.assign(nf + 1, 0);
  size_t nblk = 0;
  for (int r = 0; r < nf; r++) {
    nblk += (size_t)(r - P.first[r] + 1);
    if (49 * nblk > 0x7fffffffULL) return false;  // block offsets are 32-bit
    P.boff[r + 1] = (int32_t)nblk;
  }
  P.nblk = nblk;
  std::vector<int32_t> cptr(nf + 1, 0), crow(nblk - nf);
  for (int r = 0; r < nf; r++)
    for (int c = P.first[r]; c < r; c++) cptr[c + 1]++;
  for (int c = 0; c < nf; c++) cptr[c + 1] += cptr[c];
  {
    std::vector<int32_t> fill(cptr.begin(), cptr.end() - 1);
    for (int r = 0; r < nf; r++)
      for (int c = P.first[r]; c < r; c++) crow[fill[c]++] = r;
  }
  auto put = [&](const std::vector<int32_t>& v) {
    const size_t o = P.ints.size();
    P.ints.insert(P.ints.end(), v.begin(), v.end());
    P.ints.resize((P.ints.size() + 63) & ~(size_t)63);
    return o;
  };
  std::vector<int32_t> ev0(p.edge_v0, p.edge_v0 + E), ev1(p.edge_v1, p.edge_v1 + E), kind(E);
  for (int e = 0; e < E; e++) kind[e] = p.edge_kind[e];
  P.o_ev0 = put(ev0); P.o_ev1 = put(ev1); P.o_kind = put(kind); P.o_hidx = put(hidx); P.o_hv = put(hv);
  P.o_vptr = put(vptr); P.o_vinc = put(vinc); P.o_prow = put(prow); P.o_pcol = put(pcol); P.o_pptr = put(pptr);
  P.o_pinc = put(pinc); P.o_first = put(P.first); P.o_boff = put(P.boff); P.o_cptr = put(cptr); P.o_crow = put(crow);
  return true;
}

// the device arena behind one call: the structure, then the work arrays
struct Layout {
  size_t o_ints, o_meas, o_est, o_bak, o_T, o_H, o_L, o_dd, o_b, o_x, o_y, o_chain, o_stats, o_dbg, end;
};
Layout make_layout(const Plan& P, size_t base, bool debug) {
  Layout L;
  size_t o = base;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += scratch_align(bytes ? bytes : 8);
    return at;
  };
  const size_t E = (size_t)P.E, N = (size_t)P.N, n = (size_t)P.n;
  L.o_ints = take(P.ints.size() * 4);
  L.o_meas = take(E * 64);
  L.o_est = take(n * 64);
  L.o_bak = take(n * 64);
  L.o_T = take(E * kT * 8);
  L.o_H = take(P.nblk * 49 * 8);
  L.o_L = take(P.nblk * 49 * 8);
  L.o_dd = take(N * 8);
  L.o_b = take(N * 8);
  L.o_x = take(N * 8);
  L.o_y = take(N * 8);
  L.o_chain = take(std::max(E, N) * 8);
  L.o_stats = take(64);
  L.o_dbg = take(debug ? E * (7 + 49 + 49) * 8 : 8);
  L.end = o;
  return L;
}

Dev make_dev(const orbx_essential_graph_problem& p, const Plan& P, const Layout& L, uint8_t* d, bool debug) {
  Dev D;
  std::memset(&D, 0, sizeof(D));
  D.n = P.n; D.nf = P.nf; D.E = P.E; D.N = P.N; D.npairs = P.npairs;
  D.fix_scale = p.fix_scale ? 1 : 0;
  D.iterations = p.iterations;
  D.npts = p.n_points;
  D.lambda_init = p.lambda_init;
  const int32_t* I = (const int32_t*)(d + L.o_ints);
  D.ev0 = I + P.o_ev0; D.ev1 = I + P.o_ev1; D.ekind = I + P.o_kind; D.hidx = I + P.o_hidx; D.hv = I + P.o_hv;
  D.vptr = I + P.o_vptr; D.vinc = I + P.o_vinc; D.prow = I + P.o_prow; D.pcol = I + P.o_pcol; D.pptr = I + P.o_pptr;
  D.pinc = I + P.o_pinc; D.first = I + P.o_first; D.boff = I + P.o_boff; D.cptr = I + P.o_cptr; D.crow = I + P.o_crow;
  D.meas = (double*)(d + L.o_meas); D.est = (double*)(d + L.o_est); D.bak = (double*)(d + L.o_bak);
  D.T = (double*)(d + L.o_T); D.Henv = (double*)(d + L.o_H); D.Lenv = (double*)(d + L.o_L);
  D.dd = (double*)(d + L.o_dd); D.b = (double*)(d + L.o_b); D.x = (double*)(d + L.o_x); D.y = (double*)(d + L.o_y);
  D.chain = (double*)(d + L.o_chain); D.stats = (double*)(d + L.o_stats);
  if (debug) {
    D.dbg_err = (double*)(d + L.o_dbg);
    D.dbg_J0 = D.dbg_err + 7 * (size_t)P.E;
    D.dbg_J1 = D.dbg_J0 + 49 * (size_t)P.E;
  }
  return D;
}

// the structure upload, the zeroed envelope, the measurements
hipError_t enqueue_setup(const Plan& P, const Layout& L, const Dev& D, uint8_t* d, const void* ints_src, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(d + L.o_ints, ints_src, P.ints.size() * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d + L.o_H, 0, scratch_align(P.nblk * 49 * 8), st);
  if (e == hipSuccess) {
    const int m = std::max(P.E, P.n);
    hipLaunchKernelGGL(k_eg_measure, dim3((m + 255) / 256), dim3(256), 0, st, D);
    e = hipGetLastError();
  }
  return e;
}

hipError_t enqueue_run(const Dev& D, hipStream_t st) {
  hipLaunchKernelGGL(k_eg_lm, dim3(1), dim3(BS), 0, st, D);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    const int m = std::max(D.n, D.npts);
    hipLaunchKernelGGL(k_eg_finish, dim3((m + 255) / 256), dim3(256), 0, st, D);
    e = hipGetLastError();
  }
  return e;
}

// a host-form session: the plan, a scratch lease, the problem's pose tables staged and uploaded
struct HostRun {
  Plan P;
  Layout L;
  Dev D;
  ScratchGuard g;
  size_t in_bytes = 0, o_scw = 0, o_snc = 0, o_xw = 0, o_pref = 0, o_h_ints = 0;
  explicit HostRun(int device) : g(device) {}
  // device: [inputs][arena][extra]; pinned host: [inputs][ints][extra]
  orbx_status open(const orbx_essential_graph_problem& p, bool debug, size_t extra, size_t* o_extra_d,
                   size_t* o_extra_h) {
    if (!make_plan(p, P)) return ORBX_ERR_CAPACITY;
    const size_t n = (size_t)p.n_vertices, m = (size_t)p.n_points;
    o_scw = 0;
    o_snc = o_scw + scratch_align(n * 64);
    o_xw = o_snc + scratch_align(n * 64);
    o_pref = o_xw + scratch_align(m * 12 + 8);
    in_bytes = o_pref + scratch_align(m * 4 + 8);
    L = make_layout(P, in_bytes, debug);
    o_h_ints = in_bytes;
    *o_extra_d = L.end;
    *o_extra_h = o_h_ints + scratch_align(P.ints.size() * 4);
    const size_t readback = debug ? L.end - L.o_meas : 0;  // the linearisation probe reads the arena back
    if (!g.l || g.l->reserve(*o_extra_d + extra, *o_extra_h + extra + readback) != hipSuccess) return ORBX_ERR_HIP;
    uint8_t* h = g.l->h;
    std::memcpy(h + o_scw, p.Scw, n * 64);
    std::memcpy(h + o_snc, p.Snc, n * 64);
    if (m && p.Xw && p.point_ref) {
      std::memcpy(h + o_xw, p.Xw, m * 12);
      std::memcpy(h + o_pref, p.point_ref, m * 4);
    }
    std::memcpy(h + o_h_ints, P.ints.data(), P.ints.size() * 4);
    uint8_t* d = g.l->d;
    D = make_dev(p, P, L, d, debug);
    D.Scw = (const double*)(d + o_scw);
    D.Snc = (const double*)(d + o_snc);
    D.Xw = (const float*)(d + o_xw);
    D.pref = (const int32_t*)(d + o_pref);
    hipError_t e = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, g.l->st);
    if (e == hipSuccess) e = enqueue_setup(P, L, D, d, h + o_h_ints, g.l->st);
    return e == hipSuccess ? ORBX_OK : ORBX_ERR_HIP;
  }
};

}  // namespace essgraph
}  // namespace orbx

// ------------------------------------------------------------------ C ABI
using namespace orbx::essgraph;

extern "C" void orbx_sim3_from_tcw(const float Tcw[12], double out[8]) {
  double R[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[3 * r + c] = (double)Tcw[4 * r + c];
  const orbx::lm::Quat q = orbx::lm::mat2q(R);
  out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
  for (int r = 0; r < 3; r++) out[4 + r] = (double)Tcw[4 * r + 3];
  out[7] = 1.0;
}

static orbx_status run_host(const orbx_essential_graph_problem* p, const orbx_essential_graph_result* res, int device,
                            double* phase_ms, long long* blocks) {
  if (!p || !res || !res->Scw_out || !res->Tcw_out || (p->n_points > 0 && !res->Xw_out)) return ORBX_ERR_ARG;
  const orbx_status chk = check(*p, true);
  if (chk != ORBX_OK) return chk;
  const orbx_status dv = orbx::select_device(device);
  if (dv != ORBX_OK) return dv;
  const size_t n = (size_t)p->n_vertices, m = (size_t)p->n_points;
  const size_t r_scw = 0, r_tcw = r_scw + orbx::scratch_align(n * 64), r_xw = r_tcw + orbx::scratch_align(n * 48),
               r_st = r_xw + orbx::scratch_align(m * 12 + 8), r_tk = r_st + 32, r_end = r_st + 256;
  HostRun R(device);
  size_t od = 0, oh = 0;
  const orbx_status op = R.open(*p, false, r_end, &od, &oh);
  if (op != ORBX_OK) return op;
  uint8_t* d = R.g.l->d + od;
  uint8_t* h = R.g.l->h + oh;
  R.D.Scw_out = (double*)(d + r_scw);
  R.D.Tcw_out = (float*)(d + r_tcw);
  R.D.Xw_out = (float*)(d + r_xw);
  R.D.o_chi0 = (double*)(d + r_st);
  R.D.o_chi1 = (double*)(d + r_st + 8);
  R.D.o_iterations = (int32_t*)(d + r_st + 16);
  R.D.o_trials = (int32_t*)(d + r_st + 20);
  R.D.o_fail = (int32_t*)(d + r_st + 24);
  hipStream_t st = R.g.l->st;
  hipError_t e = enqueue_run(R.D, st);
  if (e == hipSuccess && phase_ms)  // the LM kernel's phase ticks ride in the result block's tail
    e = hipMemcpyAsync(d + r_tk, R.D.stats + 5, 24, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h, d, r_end, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = R.g.l->sync();
  if (e != hipSuccess) return ORBX_ERR_HIP;
  std::memcpy(res->Scw_out, h + r_scw, n * 64);
  std::memcpy(res->Tcw_out, h + r_tcw, n * 48);
  if (m) std::memcpy(res->Xw_out, h + r_xw, m * 12);
  if (res->chi2_initial) std::memcpy(res->chi2_initial, h + r_st, 8);
  if (res->chi2_final) std::memcpy(res->chi2_final, h + r_st + 8, 8);
  if (res->iterations) std::memcpy(res->iterations, h + r_st + 16, 4);
  if (res->trials) std::memcpy(res->trials, h + r_st + 20, 4);
  if (res->solver_failures) std::memcpy(res->solver_failures, h + r_st + 24, 4);
  if (phase_ms) {
    double ticks[3];
    std::memcpy(ticks, h + r_tk, 24);
    for (int k = 0; k < 3; k++) phase_ms[k] = ticks[k] * 1e-5;  // wall_clock64 counts at 100 MHz
  }
  if (blocks) *blocks = (long long)R.P.nblk;
  return ORBX_OK;
}

extern "C" orbx_status orbx_optimize_essential_graph(const orbx_essential_graph_problem* p,
                                                     const orbx_essential_graph_result* res, int device) {
  return run_host(p, res, device, nullptr, nullptr);
}

extern "C" int orbx_debug_essgraph_phases(const orbx_essential_graph_problem* p, const orbx_essential_graph_result* res,
                                          double phase_ms[3], long long* envelope_blocks, int device) {
  if (!phase_ms) return ORBX_ERR_ARG;
  return run_host(p, res, device, phase_ms, envelope_blocks);
}

extern "C" orbx_status orbx_optimize_essential_graph_device(const orbx_essential_graph_problem* p,
                                                            const orbx_essential_graph_result* res, void* stream) {
  if (!p || !res || !res->Scw_out || !res->Tcw_out || (p->n_points > 0 && !res->Xw_out)) return ORBX_ERR_ARG;
  const orbx_status chk = check(*p, false);
  if (chk != ORBX_OK) return chk;
  Plan P;
  if (!make_plan(*p, P)) return ORBX_ERR_CAPACITY;
  const Layout L = make_layout(P, 0, false);
  hipStream_t st = (hipStream_t)stream;
  return orbx::with_stream_block(L.end, st, [&](uint8_t* d) {
    Dev D = make_dev(*p, P, L, d, false);
    D.Scw = p->Scw; D.Snc = p->Snc; D.Xw = p->Xw; D.pref = p->point_ref;
    D.Scw_out = res->Scw_out; D.Tcw_out = res->Tcw_out; D.Xw_out = res->Xw_out;
    D.o_iterations = res->iterations; D.o_trials = res->trials; D.o_chi0 = res->chi2_initial;
    D.o_chi1 = res->chi2_final; D.o_fail = res->solver_failures;
    // pageable source: hipMemcpyAsync returns once P.ints is staged, so the plan may go
    const hipError_t e = enqueue_setup(P, L, D, d, P.ints.data(), st);
    return e != hipSuccess ? e : enqueue_run(D, st);
  });
}

// ------------------------------------------------------------------ debug probes (orbx_debug.h)
static int debug_unary(const double* x, int n, double* y, int device, int what) {
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
    hipLaunchKernelGGL(k_debug_unary, dim3((n + 255) / 256), dim3(256), 0, S.stream(), (const double*)S.dev(s_x), n,
                       S.dev(s_y), what);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = S.download();
  if (e == hipSuccess) e = S.sync();
  if (e != hipSuccess) return ORBX_ERR_HIP;
  S.fetch(s_y, y, (size_t)n);
  return ORBX_OK;
}
extern "C" int orbx_debug_log(const double* x, int n, double* y, int device) { return debug_unary(x, n, y, device, 0); }
extern "C" int orbx_debug_acos(const double* x, int n, double* y, int device) { return debug_unary(x, n, y, device, 1); }

extern "C" int orbx_debug_sim3_log(const double* S, int n, double* out, int32_t* branch, int device) {
  if (n < 0 || (n > 0 && (!S || !out))) return ORBX_ERR_ARG;
  const orbx_status dv = orbx::select_device(device);
  if (dv != ORBX_OK) return dv;
  if (n == 0) return ORBX_OK;
  orbx::Staging G(device);
  const auto s_S = G.in(S, (size_t)n * 8);
  const auto s_out = G.out<double>((size_t)n * 7);
  const auto s_br = G.out<int32_t>((size_t)n);
  const orbx_status cs = G.commit();
  if (cs != ORBX_OK) return cs;
  hipError_t e = G.upload(orbx::Staging::Outputs::skipped);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_debug_sim3_log, dim3((n + 255) / 256), dim3(256), 0, G.stream(), (const double*)G.dev(s_S), n,
                       G.dev(s_out), G.dev(s_br));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = G.download();
  if (e == hipSuccess) e = G.sync();
  if (e != hipSuccess) return ORBX_ERR_HIP;
  G.fetch(s_out, out, (size_t)n * 7);
  G.fetch(s_br, branch, (size_t)n);
  return ORBX_OK;
}

extern "C" int orbx_debug_essgraph_linearize(const orbx_essential_graph_problem* p, double* meas, double* err,
                                             double* J0, double* J1, double* H, double* b, int device) {
  if (!p) return ORBX_ERR_ARG;
  orbx_essential_graph_problem q = *p;
  q.n_points = 0;
  const orbx_status chk = check(q, true);
  if (chk != ORBX_OK) return chk;
  const orbx_status dv = orbx::select_device(device);
  if (dv != ORBX_OK) return dv;
  HostRun R(device);
  size_t od = 0, oh = 0;
  orbx_status op = R.open(q, true, 0, &od, &oh);
  if (op != ORBX_OK) return op;
  // the read-back: everything from the measurements to the probe block, staged behind the inputs
  const size_t span = R.L.end - R.L.o_meas;
  hipStream_t st = R.g.l->st;
  hipLaunchKernelGGL(k_eg_linearize, dim3(1), dim3(BS), 0, st, R.D);
  hipError_t e = hipGetLastError();
  uint8_t* h = R.g.l->h + oh;
  if (e == hipSuccess) e = hipMemcpyAsync(h, R.g.l->d + R.L.o_meas, span, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = R.g.l->sync();
  if (e != hipSuccess) return ORBX_ERR_HIP;
  const size_t E = (size_t)R.P.E, N = (size_t)R.P.N;
  auto at = [&](size_t o) { return (const double*)(h + (o - R.L.o_meas)); };
  if (meas) std::memcpy(meas, at(R.L.o_meas), E * 64);
  if (err) std::memcpy(err, at(R.L.o_dbg), E * 56);
  if (J0) std::memcpy(J0, at(R.L.o_dbg) + 7 * E, E * 49 * 8);
  if (J1) std::memcpy(J1, at(R.L.o_dbg) + 56 * E, E * 49 * 8);
  if (b) std::memcpy(b, at(R.L.o_b), N * 8);
  if (H) {
    std::memset(H, 0, N * N * 8);
    const double* env = at(R.L.o_H);
    for (int i = 0; i < R.P.N; i++) {
      const int r = i / 7, il = i % 7, f = R.P.first[r], Wd = 7 * (r - f + 1);
      const double* row = env + 49 * (size_t)R.P.boff[r] + (size_t)il * Wd;
      for (int j = 7 * f; j <= i; j++) H[(size_t)i * N + j] = H[(size_t)j * N + i] = row[j - 7 * f];
    }
  }
  return ORBX_OK;
}

extern "C" int orbx_debug_essgraph_solve(const orbx_essential_graph_problem* p, const double* H, const double* b,
                                         double lambda, double* x, int32_t* ok, int device) {
  if (!p || !H || !b || !x || !ok) return ORBX_ERR_ARG;
  orbx_essential_graph_problem q = *p;
  q.n_points = 0;
  const orbx_status chk = check(q, true);
  if (chk != ORBX_OK) return chk;
  const orbx_status dv = orbx::select_device(device);
  if (dv != ORBX_OK) return dv;
  Plan P;
  if (!make_plan(q, P)) return ORBX_ERR_CAPACITY;
  const size_t N = (size_t)P.N, envb = orbx::scratch_align(P.nblk * 49 * 8), nb = orbx::scratch_align(N * 8);
  const Layout L = make_layout(P, 0, false);
  const size_t intb = orbx::scratch_align(P.ints.size() * 4);
  orbx::ScratchGuard g(device);
  if (!g.l || g.l->reserve(L.end, envb + nb + intb + 256) != hipSuccess) return ORBX_ERR_HIP;
  uint8_t* h = g.l->h;
  double* env = (double*)h;
  std::memset(env, 0, envb);
  for (int i = 0; i < P.N; i++) {
    const int r = i / 7, il = i % 7, f = P.first[r], Wd = 7 * (r - f + 1);
    double* row = env + 49 * (size_t)P.boff[r] + (size_t)il * Wd;
    for (int j = 7 * f; j <= i; j++) row[j - 7 * f] = H[(size_t)i * N + j];
  }
  std::memcpy(h + envb, b, N * 8);
  std::memcpy(h + envb + nb, P.ints.data(), P.ints.size() * 4);
  uint8_t* d = g.l->d;
  const Dev D = make_dev(q, P, L, d, false);
  hipStream_t st = g.l->st;
  hipError_t e = hipMemcpyAsync(d + L.o_ints, h + envb + nb, P.ints.size() * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d + L.o_H, h, P.nblk * 49 * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d + L.o_b, h + envb, N * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_eg_solve, dim3(1), dim3(BS), 0, st, D, lambda);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h, d + L.o_x, N * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h + nb, d + L.o_stats, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = g.l->sync();
  if (e != hipSuccess) return ORBX_ERR_HIP;
  std::memcpy(x, h, N * 8);
  double okd;
  std::memcpy(&okd, h + nb, 8);
  *ok = okd != 0.0;
  return ORBX_OK;
}

// ba_lm.h -- LocalBundleAdjustment (localba.hip): the state update and the Levenberg-Marquardt
// control on the device.  k_ba_update / k_ba_restore (push, oplus, pop), the phase entry
// (k_ba_lm_start; batched: k_ba_dmax_many + k_ba_lm_init_many), the per-trial verdict
// (k_ba_lm_control, or fused with the errors in k_ba_errors_ctl), k_ba_lm_resume, k_ba_lm_final_many.
// The verdict's Levenberg arithmetic (gain ratio, lambda update, trial budget, the _nBad rule) is
// orbx_lm.h's lm::trial / lm::iteration_end, here with the once-rounded cube of oracle/localba.cpp.
#pragma once
#include "ba_linearize.h"
#include "orbx_lm.h"

namespace orbx {

constexpr int kUpCh = 2048;  // k_ba_update: positions per LDS chunk (48 KB)
// k_ba_update: points per block (all LBS threads form the position products): 64 points take one
// round of position products per block and four times the blocks (10.8 -> 7.4 us at config 4;
// 32 points: 7.0 us, within the spread)
constexpr int kUpPts = 64;
static_assert(kUpPts <= LBS, "one thread per point");
// back-substitution + update (push first) + LM scale, skipped when the solve failed
// (scal[2] == 0).  Blocks: the active poses first (their se3 exp chains then overlap the point
// blocks), then LBS active points per block; one LM-scale partial per block.
__device__ __forceinline__ void k_ba_update_body(const BaDev& D, double lambda) {
  if (lm_skip(D) || (int)blockIdx.x >= D.nbu) return;
  lambda = lm_lambda(D, lambda);
  // device LM: the previous trial's pop is folded in (same values as k_ba_restore).
  // Every state value is loaded into registers before any store: the X / Xbak (cq, cbak)
  // stores may alias the next loads as far as the compiler knows, which otherwise
  // serialised each load behind the previous store (one memory round trip apiece).
  const bool rej = D.lm && D.lm->rejected;
  const bool ok = D.scal[2] != 0.0;
  const int npb = (D.nposes + LBS - 1) / LBS;
  double sc = 0;
  if ((int)blockIdx.x < npb) {
    const int pi = blockIdx.x * LBS + threadIdx.x;
    if (pi < D.nposes) {
      const int c = D.pose_cam[pi];
      double u[6], bp[6];
      for (int r = 0; r < 6; r++) {
        u[r] = D.xp[6 * pi + r];
        bp[r] = D.bp[6 * pi + r];
      }
      double q4[4], t3[3];
      if (rej) {
        for (int r = 0; r < 4; r++) q4[r] = D.cbak[7 * c + r];
        for (int r = 0; r < 3; r++) t3[r] = D.cbak[7 * c + 4 + r];
      } else {
        for (int r = 0; r < 4; r++) q4[r] = D.cq[4 * c + r];
        for (int r = 0; r < 3; r++) t3[r] = D.ct[3 * c + r];
      }
      if (ok) {
        for (int r = 0; r < 6; r++) sc += u[r] * (lambda * u[r] + bp[r]);
        for (int r = 0; r < 4; r++) D.cbak[7 * c + r] = q4[r];
        for (int r = 0; r < 3; r++) D.cbak[7 * c + 4 + r] = t3[r];
        const SE3d E = se3_exp(u);
        const Quat q = {q4[0], q4[1], q4[2], q4[3]};
        double rt[3];
        qrot(E.q, t3, rt);
        Quat nq = qmul(E.q, q);
        qnormalize(nq);
        D.cq[4 * c] = nq.x;
        D.cq[4 * c + 1] = nq.y;
        D.cq[4 * c + 2] = nq.z;
        D.cq[4 * c + 3] = nq.w;
        for (int r = 0; r < 3; r++) D.ct[3 * c + r] = E.t[r] + rt[r];
      } else if (rej) {
        for (int r = 0; r < 4; r++) D.cq[4 * c + r] = q4[r];
        for (int r = 0; r < 3; r++) D.ct[3 * c + r] = t3[r];
      }
    }
  } else {
    const int i0 = (blockIdx.x - npb) * kUpPts, i = i0 + threadIdx.x, i1 = min(i0 + kUpPts, D.npa);
    const bool pt = (int)threadIdx.x < kUpPts && i < D.npa;
    const int ic = pt ? i : i0;  // (i0 < npa in a point block) loads stay in range
    // everything that depends on neither the solve's flag nor the LM state, issued first
    const int p = D.pt_id[ic];
    const int ka = D.pt_off[ic], kz = pt ? D.pt_off[ic + 1] : ka;
    const int kb = D.pt_off[i0], ke = D.pt_off[i1];
    double c[3], bl[3], Di[9];
    for (int r = 0; r < 3; r++) c[r] = bl[r] = D.bl[3 * ic + r];
    for (int r = 0; r < 9; r++) Di[r] = D.Dinv[9 * (size_t)ic + r];
    const double* from = rej ? D.Xbak : D.X;
    const double X0[3] = {from[3 * p], from[3 * p + 1], from[3 * p + 2]};
    // b_l - sum_k Hpl_k^T x_c(k): the per-position products H_pl^T x_c are formed by all the
    // block's threads at once (4 positions per thread per round, every load issued before the
    // arithmetic) and staged in LDS; each point's thread then subtracts its positions' products
    // in position order.  (A thread per point walking its own positions paid two dependent
    // memory round trips per position.)  Unused when the solve failed.
    __shared__ double sq[kUpCh * 3];
    for (int base = kb; base < ke; base += kUpCh) {  // block-uniform
      const int n = min(kUpCh, ke - base);
      for (int u0 = threadIdx.x; u0 < n; u0 += 4 * LBS) {
        int ci[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
          const int u = u0 + s * LBS;
          ci[s] = u < n ? D.pcam[base + u] : -1;
        }
        double B[4][18], x[4][6];
#pragma unroll
        for (int s = 0; s < 4; s++) {
          const int u = min(u0 + s * LBS, n - 1);
          const double* h = D.Hpl + 18 * (size_t)(base + u);
          const double* xc = D.xp + 6 * max(ci[s], 0);
#pragma unroll
          for (int j = 0; j < 18; j++) B[s][j] = h[j];
#pragma unroll
          for (int r = 0; r < 6; r++) x[s][r] = xc[r];
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
          const int u = u0 + s * LBS;
          if (u < n) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
              double q = 0;
#pragma unroll
              for (int r = 0; r < 6; r++) q += B[s][3 * r + j] * x[s][r];
              sq[3 * u + j] = ci[s] >= 0 ? q : 0.0;  // fixed camera: no term
            }
          }
        }
      }
      __syncthreads();
      for (int k = max(ka, base); k < min(kz, base + n); k++)
#pragma unroll
        for (int j = 0; j < 3; j++) c[j] -= sq[3 * (k - base) + j];
      __syncthreads();
    }
    if (pt) {
      if (ok) {
        double x[3];
        for (int r = 0; r < 3; r++) x[r] = Di[3 * r] * c[0] + Di[3 * r + 1] * c[1] + Di[3 * r + 2] * c[2];
        for (int r = 0; r < 3; r++) sc += x[r] * (lambda * x[r] + bl[r]);
        for (int r = 0; r < 3; r++) {
          D.Xbak[3 * p + r] = X0[r];
          D.X[3 * p + r] = X0[r] + x[r];
        }
      } else if (rej) {
        for (int r = 0; r < 3; r++) D.X[3 * p + r] = X0[r];
      }
    }
  }
  block_partial(sc, D.scal + 8 + 2 * D.nbe);
}
__global__ __launch_bounds__(LBS) void k_ba_update(BaDev D, double lambda) { k_ba_update_body(D, lambda); }
__global__ __launch_bounds__(LBS) void k_ba_update_many(const BaDev* __restrict__ Ds, double lambda) {
  k_ba_update_body(Ds[blockIdx.z], lambda);
}

__device__ __forceinline__ void k_ba_restore_body(const BaDev& D) {
  if (D.lm && !D.lm->rejected) return;  // (a refresh always follows a rejected trial)
  const int i = blockIdx.x * LBS + threadIdx.x;
  if (i < D.npa) {
    const int p = D.pt_id[i];
    const double v[3] = {D.Xbak[3 * p], D.Xbak[3 * p + 1], D.Xbak[3 * p + 2]};  // loads before stores
    for (int r = 0; r < 3; r++) D.X[3 * p + r] = v[r];
  } else if (i < D.npa + D.nposes) {
    const int c = D.pose_cam[i - D.npa];
    double v[7];
    for (int r = 0; r < 7; r++) v[r] = D.cbak[7 * c + r];
    for (int r = 0; r < 4; r++) D.cq[4 * c + r] = v[r];
    for (int r = 0; r < 3; r++) D.ct[3 * c + r] = v[4 + r];
  }
}
__global__ __launch_bounds__(LBS) void k_ba_restore(BaDev D) { k_ba_restore_body(D); }
__global__ __launch_bounds__(LBS) void k_ba_restore_many(const BaDev* __restrict__ Ds) {
  k_ba_restore_body(Ds[blockIdx.z]);
}

// optimize() entry: lambda = tau * max diag(H) (computeLambdaInit), chi of
// the linearised state from errors slot 0 (block partials, fixed_sum_wave's tree).
__device__ __forceinline__ void k_ba_lm_init_body(const BaDev& D, int iterations) {
  LmState* L = const_cast<LmState*>(D.lm);
  const double a = fixed_sum_wave(D.scal + 8, D.nbe);
  if (threadIdx.x != 0) return;
  lm::Step s;
  lm::start(s, 1e-5 * D.scal[3]);
  L->lambda = s.lambda;
  L->ni = s.ni;
  L->currentChi = L->iniChi = a;
  L->nBad = s.nBad;
  L->it = L->qmax = L->trials = 0;
  L->relin = 0;  // linearised by the entry launches
  L->rejected = 0;
  L->iterations = iterations;
  L->stopped = 0;  // the host polled the flag just before this phase
  L->refresh = 0;
  L->done = iterations <= 0 ? 1 : 0;
  L->ticket = 0;
}
// A phase's entry after k_ba_cam_sum (single-problem device LM): k_ba_cam_fin, the lambda init (the
// max of |H_jj| over points and poses -> scal[3], a 1024-wide tree: max is order-free) and the LM
// state init in one launch; the batched driver runs k_ba_cam_fin_many, k_ba_dmax_many and
// k_ba_lm_init_many
__global__ __launch_bounds__(1024) void k_ba_lm_start(BaDev D, int iterations) {
  __shared__ double wmax[16];
  double acc = 0.0;
  for (int i = threadIdx.x; i < D.npa; i += 1024) acc = fmax(acc, D.dmax_p[i]);
  // k_ba_cam_fin's finalisation of the entry's pose sums: item (pose, j) sums the chunk partials of
  // its upper-triangle / rhs entry in chunk order (Hpp both triangles, bp); the diagonal entries'
  // |H_jj| join the lambda-init maximum here, and after the barrier each pose's thread takes its own
  // maximum from the six diagonal entries this block just wrote
  const int S = D.gsplit;
  auto csum = [&](int ci, int q) {  // chunk order; loads in groups of 8 (clamped) before their adds
    double t = 0;
    for (int c0 = 0; c0 < S; c0 += 8) {
      double v[8];
#pragma unroll
      for (int e = 0; e < 8; e++) v[e] = D.gpart[((size_t)ci * S + min(c0 + e, S - 1)) * 27 + q];
#pragma unroll
      for (int e = 0; e < 8; e++)
        if (c0 + e < S) t += v[e];
    }
    return t;
  };
  for (int it = threadIdx.x; it < D.nposes * 42; it += 1024) {
    const int ci = it / 42, j = it - ci * 42;
    if (j < 36) {
      const int r = min(j / 6, j % 6), c = max(j / 6, j % 6);
      const double v = csum(ci, r * 6 - (r * (r - 1)) / 2 + (c - r));
      D.Hpp[36 * ci + j] = v;
      if (j / 6 == j % 6) acc = fmax(acc, fabs(v));
    } else {
      D.bp[6 * ci + (j - 36)] = csum(ci, 21 + (j - 36));
    }
  }
  // the maximum over the block: wave maxima by lane exchanges, then the 16 of them (max is order-free)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc = fmax(acc, __shfl_xor(acc, o, 64));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = acc;
  __syncthreads();  // (also orders the Hpp stores above before the per-pose reads below)
  for (int ci = threadIdx.x; ci < D.nposes; ci += 1024) {
    double m = 0;
    for (int r = 0; r < 6; r++) m = fmax(m, fabs(D.Hpp[36 * ci + 7 * r]));
    D.dmax_c[ci] = m;
  }
  if (threadIdx.x >= 64) return;
  if (threadIdx.x == 0) {
    double m = wmax[0];
    for (int w = 1; w < 16; w++) m = fmax(m, wmax[w]);
    D.scal[3] = m;  // (read back below by the same thread)
  }
  k_ba_lm_init_body(D, iterations);
}
__global__ __launch_bounds__(64) void k_ba_lm_init_many(const BaDev* __restrict__ Ds, int iterations) {
  k_ba_lm_init_body(Ds[blockIdx.z], iterations);
}

// One LM trial's verdict (OptimizationAlgorithmLevenberg::solve, the
// reference's decisions in the same sequence as the host loop of
// LocalBA::optimize): chi and LM scale summed from the block partials by
// fixed_sum_wave (its lane-strided tree, where the host loop adds them in
// index order: the low bits of the two sums differ), accept (lambda *= max(1/3, min(2/3, 1-(2rho-1)^3))) or reject
// (lambda *= ni, ni *= 2, restore), then the iteration bookkeeping: the
// <= 10 trial budget, rho == 0, the _nBad rule and the stop flag.
template <bool coh = false>
__device__ __forceinline__ void k_ba_lm_control_body(const BaDev& D, DevStop stop) {
  LmState* L = const_cast<LmState*>(D.lm);
  const int nbu = D.nbu;
  if (L->done) return;  // uniform; a finished phase keeps `rejected` for the final restore
  // the flag's host-memory read is issued first, so its latency hides behind the sums (one read
  // serves both of the loop's polls below; a flag raised after it is seen at the next trial)
  // (thread 0 alone reads it: the verdict below is thread 0's)
  const bool st = threadIdx.x == 0 && (stop() || (D.raise_after >= 0 && L->trials >= D.raise_after));  // (+ test hook)
  const double* p = D.scal + 8;
  double b, u;
  fixed_sum2_wave<coh>(p + D.nbe, D.nbe, p + 2 * D.nbe, nbu, b, u);
  if (threadIdx.x != 0) return;
  L->rejected = 0;
  const bool ok2 = D.scal[2] != 0.0;
  if (L->qmax == 0) L->iniChi = L->currentChi;
  L->trials++;
  // the shared step on a copy of the state's Levenberg fields (LmState's layout is the host's and the
  // capture path's; rho lives for this call only).  Its min / max take the operands in std::min's and
  // std::max's order, as the oracle does: should the cube overflow (rho beyond 1e102, i.e. an LM scale
  // of exactly -1e-3) the factor is the oracle's 1/3, where this kernel's former operand order gave 2/3.
  lm::Step s = {L->lambda, L->ni, L->currentChi, L->iniChi, 0.0, L->qmax, L->nBad};
  const lm::Verdict v = lm::trial<lm::Cube::kRounded>(s, b, u, ok2);
  L->lambda = s.lambda;
  L->ni = s.ni;
  L->currentChi = s.currentChi;
  L->qmax = s.qmax;
  if (!v.accept && ok2) L->rejected = 1;
  if (v.go && !st) {  // another trial of this iteration
    L->relin = 0;
    return;
  }
  L->it++;
  const bool brk = lm::iteration_end(s);
  L->nBad = s.nBad;
  L->qmax = 0;
  const bool st2 = !brk && L->it < L->iterations && st;
  L->stopped = st || st2;
  L->done = (brk || L->it >= L->iterations || st2) ? 1 : 0;
  L->relin = L->done ? 0 : 1;
  if (!L->done && L->rejected) {
    // rho was NaN: the iteration ended on a rejection and the phase goes on.  g2o pops the
    // trial and its next iteration recomputes the errors at the restored state; pause the
    // phase until the host has queued exactly that (restore, errors, k_ba_lm_resume).
    L->refresh = 1;
    L->done = 1;
  }
}

// Resume a phase paused for a refresh: chi of the recomputed errors (slot 0, summed by
// fixed_sum_wave's tree; the host loop's computeActiveErrors + activeRobustChi2 adds them in
// index order) becomes the iteration's starting chi.
__device__ __forceinline__ void k_ba_lm_resume_body(const BaDev& D) {
  LmState* L = const_cast<LmState*>(D.lm);
  if (!L->refresh) return;
  const double a = fixed_sum_wave(D.scal + 8, D.nbe);
  if (threadIdx.x != 0) return;
  L->currentChi = a;
  L->rejected = 0;
  L->refresh = 0;
  L->done = 0;
  L->relin = 1;
}
__global__ __launch_bounds__(64) void k_ba_lm_resume(BaDev D) { k_ba_lm_resume_body(D); }
__global__ __launch_bounds__(64) void k_ba_lm_resume_many(const BaDev* __restrict__ Ds) {
  k_ba_lm_resume_body(Ds[blockIdx.z]);
}
// A trial's k_ba_errors(D, 1, 1) and k_ba_lm_control in one launch (single-problem device LM): every
// block's thread 0 stores its chi partial (agent scope) and then takes a ticket with an agent-scope
// release RMW; the block whose ticket is the last one issues one agent-scope acquire fence after
// it and has thereby acquired every other block's release (the RMWs form one release sequence),
// i.e. every partial store happens-before its reads (the block barrier carries that to the rest of
// the block).  That block runs the verdict (wave 0 works, the other waves only pass the
// barriers).  Same partials, same order, same arithmetic as the two launches k_ba_errors +
// k_ba_lm_control, which are the default (debug option fused_ctl selects this one; tests compare
// the two bit for bit): the per-block release costs more than the dispatch it saves.
__global__ __launch_bounds__(LBS) void k_ba_errors_ctl(BaDev D, DevStop stop) {
  if (!k_ba_errors_body<true>(D, 1, 1)) return;
  __shared__ int last;
  if (threadIdx.x == 0) {
    unsigned* tk = &const_cast<LmState*>(D.lm)->ticket;
    // release RMW in every block (the RMWs form one release sequence); only the block that reads the
    // last ticket needs the acquire, as a fence after its RMW (the other blocks skip the L2 invalidate)
    last = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(D.nbe - 1);
    if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (last) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last) return;  // (uniform per block)
  k_ba_lm_control_body<true>(D, stop);
}
// The two-launch form's verdict (the default): after k_ba_errors(D, 1, 1), one wave.
__global__ __launch_bounds__(64) void k_ba_lm_control(BaDev D, DevStop stop) { k_ba_lm_control_body(D, stop); }
__global__ __launch_bounds__(64) void k_ba_lm_control_many(const BaDev* __restrict__ Ds, DevStop stop) {
  k_ba_lm_control_body(Ds[blockIdx.z], stop);
}

// Batched driver helpers (one block per problem, blockIdx.z): the lambda-init
// maximum of |H_jj| (k_ba_lm_start's partition and order) and the phase's final
// chi from errors slot 0 (summed in block order, like the host readback).
__global__ __launch_bounds__(1024) void k_ba_dmax_many(const BaDev* __restrict__ Ds) {
  const BaDev& D = Ds[blockIdx.z];
  __shared__ double sm[1024];
  const int n = D.npa + D.nposes;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) acc = fmax(acc, D.dmax_p[i]);
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) D.scal[3] = sm[0];
}
__global__ __launch_bounds__(64) void k_ba_lm_final_many(const BaDev* __restrict__ Ds) {
  const BaDev& D = Ds[blockIdx.z];
  const double a = index_order_sum_wave(D.scal + 8, D.nbe);
  if (threadIdx.x == 0) const_cast<LmState*>(D.lm)->final_chi = a;
}

}  // namespace orbx

// ba_types.h -- LocalBundleAdjustment (localba.hip): what every part of the solver shares.  The
// handle's debug options, the stop flag (host and device views), the device LM state, the problem
// descriptor every kernel takes (BaDev), the gates of the device LM loop, and the block sizes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/orbx.h"
#include "../../include/orbx_debug.h"
#include "orbx_device.h"

namespace orbx {

// Debug / test options of the solver handle running on this thread (orbx_debug_ba_options); the
// production default is all-off.  Set for the duration of an orbx_ba_run* call (BaOptScope).
constexpr orbx_ba_debug_options kBaOptsDefault = {ORBX_BA_LDLT_AUTO, -1, -1, 0, 0};
inline thread_local const orbx_ba_debug_options* t_ba_opts = nullptr;
inline const orbx_ba_debug_options& ba_opts() { return t_ba_opts ? *t_ba_opts : kBaOptsDefault; }
struct BaOptScope {  // the handle's options for this call on this thread
  const orbx_ba_debug_options* prev;
  explicit BaOptScope(const orbx_ba_debug_options* o) : prev(t_ba_opts) { t_ba_opts = o; }
  ~BaOptScope() { t_ba_opts = prev; }
};

// The reference's pbStopFlag (bool*, src/Optimizer.cc:530, set by LocalMapping::InterruptBA) or an
// int mirror of it; polled before the run and between LM trials (SparseOptimizer::terminate()).
struct StopFlag {
  const volatile int* i = nullptr;
  const volatile bool* b = nullptr;
  bool operator()() const { return (i && *i) || (b && *b); }
};

// ------------------------------------------------------------ device state
constexpr int LBS = 256;  // block size of the per-position / per-point kernels
constexpr int kCmc = 27;  // pose terms per position (see lin_pose_terms)
constexpr int kGB = 256;  // gather-block size (pose lists are split into chunks across blocks)
constexpr int kGW = kGB / 64;
constexpr int kGPpt = 2;  // ~positions per thread of a pose chunk (sets BaDev::gsplit)
constexpr int kPB = 256;  // k_ba_pair_table / k_ba_pairs block size

// Levenberg-Marquardt control of one optimize() call kept on the device
// (OptimizationAlgorithmLevenberg::solve + the _nBad rule, Appendix B of
// SURVEY): k_ba_lm_control updates it after every trial, and the trial's
// kernels read lambda and the gates from it, so a phase runs without a host
// round trip per trial.
struct LmState {
  double lambda, ni, currentChi, iniChi;
  int it, qmax, nBad, trials;
  int relin;       // the next trial starts a new iteration: linearise first
  int done;        // the phase has ended: every gated kernel returns at once
  int rejected;    // the last trial was rejected after a successful solve: restore
  int iterations;  // the phase's iteration budget
  int stopped;     // the stop flag was seen
  int refresh;     // an iteration ended on a rejected trial (rho NaN) and the phase goes on: the
                   // phase pauses (done) until the host pops the trial, recomputes the errors at
                   // the restored state and resumes (k_ba_lm_resume), as g2o's next iteration does
  double final_chi;  // batched driver: activeRobustChi2 of the stored errors at the phase end
  unsigned ticket;   // k_ba_errors_ctl: blocks of the current launch that have stored their partial
};

struct BaDev {
  int nc, np, ne;
  // cameras
  double* cq;    // nc*4 (x,y,z,w)
  double* ct;    // nc*3
  double* cbak;  // nc*7
  const double* intr;  // nc*5 fx,fy,cx,cy,bf
  int* chidx;    // nc: pose hessian index or -1
  // points
  double* X;     // np*3
  double* Xbak;  // np*3
  // edges (all)
  const int* ept;
  const int* ecam;
  const uint8_t* est;    // stereo flag
  const double* eobs;    // ne*3
  const double* einfo;  // ne
  const double* edelta; // ne
  const float* edsqr;   // ne
  uint8_t* erobust;     // ne
  double* eerr;         // ne*3
  // active edge structure (positions k = 0..na-1, point-major)
  int na;
  int* act;        // na: edge id
  int* pt_off;     // npa+1 over positions
  int* pt_id;      // npa: point id of active point i
  int npa;
  int* cam_pos;    // positions grouped by active pose
  int* cam_off;    // nposes+1
  int* pose_cam;   // nposes: camera id
  int nposes;
  int* pcam;       // na: pose index of position k (-1: fixed camera)
  int* boff;       // nblk+1: block b's slice of ptab (one slot per position of pose c1)
  int* ptab;       // per (block, c1 position): first c2 partner k2 | more<<30, or -1
  int nblk;        // nposes*(nposes+1)/2 upper-triangle Hschur blocks
  // per position
  double* Hpl;     // na*18 (6x3)
  double* ptc;     // na*12: Hll 9 + bl 3
  double* cmc;     // na*kCmc: Hpp upper triangle 21 (row-major, c >= r) + bp 6
  double* BD;      // na*18
  double* cf;      // na*6
  // per active point
  double* Hll;     // npa*9
  double* bl;      // npa*3
  double* Dinv;    // npa*9
  double* dmax_p;  // npa
  // per pose
  double* Hpp;     // nposes*36
  double* bp;      // nposes*6
  double* xp;      // nposes*6
  double* bs;      // nposes*6
  double* S;       // (6*nposes)^2
  double* Sw;      // padded LDLT work matrix when it does not fit LDS
  unsigned long long* dbg;  // optional phase timestamps (debug probe only)
  double* dmax_c;  // nposes
  int* pos_pt;     // na: active point index of position k
  int* pblk;       // nbf+1: first active point of each fused point-side block (k_ba_lin_schur), or null
  int nbf;         // fused point-side blocks (0: the unfused kernels run)
  int fused;       // device-LM launches of a problem with nbf > 0: k_ba_lin_schur does the point side
                   // (3: a phase's entry linearisation -- k_ba_linearize + k_ba_point_sum's outputs only)
                   // of iteration-start trials (k_ba_linearize / point_sum / point_schur skip them)
  int ldlt_pan;    // the reduced system goes through k_ba_ldlt_pan (else the column-step kernel): per
                   // problem, so a batch with both kinds launches both and each skips the other's
  int camfold;     // device-LM trials: k_ba_pairs' rhs blocks also sum the pose terms (k_ba_cam_sum's
                   // partials) and k_ba_schur_fin does k_ba_cam_fin's Hpp / bp (not launched)
  double* gpart;   // chunk partials of the pose-list gathers (summed by the *_fin kernels)
  double* gpose;   // posepart: nbf x nposes x kCmc -- per fused block and pose, the pose terms of the
                   // block's positions on that pose summed in position order (relinearising trials)
  int posepart;    // relinearising device-LM trials: k_ba_lin_schur writes gpose instead of the
                   // per-position pose terms, k_ba_pairs' rhs blocks sum gpose over the fused blocks
  int bdfold;      // device-LM trials of a fused problem: B D^-1 is not stored; k_ba_pairs forms it
                   // from H_pl and the point's D^-1 (the same expression, the same bits)
  int gsplit;      // chunks per pose list in the gather kernels
  int nbe;         // k_ba_errors blocks; scal[8..] holds its block partials (2 slots), then k_ba_update's
  int nbu;         // k_ba_update blocks (its LM-scale partials)
  double* scal;    // scalars: [0] chi at iteration start, [1] chi after the trial, [2] solve ok, [3] max diag, [4] LM scale
  const LmState* lm;  // device LM state: gates the trial's kernels and carries lambda (null: host control)
  // phase-end readout (set on the last k_ba_errors launch of a phase only): the launch also writes
  // its block partials, block 0 the rest of the readback block and *lm_copy, into mapped pinned
  // memory (rb_out, lm_out), so the host reads them after one event with no copy launches
  double* rb_out;
  LmState* lm_out;
  const LmState* lm_copy;
  int nan_trial;      // debug (ORBX_BA_NAN_TRIAL): this trial's chi is NaN; -1 off
  int raise_after;    // debug (ORBX_BA_RAISE_STOP_AFTER): the device raises the stop mirror after this many trials; -1 off
};

// gates of the device LM loop (uniform per launch, checked before any barrier)
__device__ inline bool lm_skip(const BaDev& D) { return D.lm && D.lm->done; }
__device__ inline bool lm_skip_lin(const BaDev& D) { return D.lm && (D.lm->done || !D.lm->relin); }
__device__ inline double lm_lambda(const BaDev& D, double lambda) { return D.lm ? D.lm->lambda : lambda; }
// The phase-2 launches queued speculatively behind phase 1's last trials (k_ba_outliers and the
// structure kernels with D.lm set): they run only if phase 1 has ended on an accepted state -- done,
// no refresh pending, no rejected trial still to pop -- and not on the stop flag (the reference
// skips phase 2 then: bDoMore, src/Optimizer.cc:764).  The host reads phase 1's state back and
// applies the same condition (spec_ran in run_local_ba).  Otherwise they return at once, and the
// host queues them again after its pop, or not at all after a stop.
__device__ inline bool spec_skip(const BaDev& D) {
  return D.lm && !(D.lm->done && !D.lm->refresh && !D.lm->rejected && !D.lm->stopped);
}

// The caller's stop flag as the device sees it (host-mapped pinned pages):
// SparseOptimizer::terminate(), polled where the host loop polls it.
struct DevStop {
  const int* i;
  const bool* b;
  __device__ bool operator()() const {
    return (i && __hip_atomic_load(i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) ||
           (b && __hip_atomic_load(reinterpret_cast<const char*>(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0);
  }
};

}  // namespace orbx

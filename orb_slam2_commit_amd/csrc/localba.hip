// localba.hip -- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:530-885)
// on g2o semantics (BlockSolver<6,3> + LinearSolverEigen + Levenberg, Huber
// kernels, two phases), FP64, device-resident.
//
// One translation unit (kernels are launched from the host code below; no relocatable device
// code), cut into headers by concern:
//   ba_types.h      debug options, stop flag, LmState, BaDev, the LM gates, block sizes
//   ba_math.h       quaternion / SE3 numerics, wave and block reductions, sums over block partials
//   ba_linearize.h  k_ba_errors, k_ba_linearize, k_ba_point_sum, k_ba_cam_sum / _fin,
//                   k_ba_point_schur, k_ba_lin_schur (the three point-side kernels fused)
//   ba_schur.h      k_ba_pair_table, k_ba_pairs, k_ba_schur_fin, the trial's fold flags
//   ba_ldlt.h       k_ba_ldlt / k_ba_ldlt_col / k_ba_ldlt_pan, k_ba_ldlt_tiled_* and LdltPlan
//   ba_lm.h         k_ba_update, k_ba_restore, k_ba_lm_*, k_ba_errors_ctl (the Levenberg step: orbx_lm.h)
//   ba_structure.h  k_ba_struct_*, k_ba_prep, k_ba_outliers, k_ba_export
//   ba_capture.h    k_ba_capture_pre / _post: the test-only capture of one trial (orbx_debug.h)
//   ba_host.h       struct LocalBA: buffers, phase structure, optimize_dev (one optimize() call)
//   ba_global.h     run_global_ba: Optimizer::GlobalBundleAdjustemnt, one optimize(n) on the same parts
//   this file       intake, write-back, run_local_ba, the batched driver, the C ABI, the LDLT probe
//
// Per LM iteration (g2o OptimizationAlgorithmLevenberg::solve):
//   k_ba_errors      computeActiveErrors + robust chi per edge (errors kept per
//                    edge exactly like g2o's _error, including after a pop)
//   k_ba_linearize   linearizeOplus + constructQuadraticForm per active edge:
//                    Hpl_e = B^T W A, point (Hll,bl) and pose (Hpp,bp) terms
//   k_ba_point_sum   Hll, bl per point (fixed edge order)
//   k_ba_cam_sum     Hpp, bp per pose: chunk partials (pose lists split over blocks)
//   k_ba_cam_fin     chunk partials -> Hpp, bp, max |Hpp_jj| (chunk order; batched driver --
//                    the single-problem entry does it inside k_ba_lm_start)
//   per trial:
//   k_ba_point_schur D = Hll + lambda I, Dinv (cofactor inverse), BD_e = Hpl_e Dinv, cf_e = Hpl_e Dinv bl
//   k_ba_pairs       chunk partials of sum_points BD_e1 Hpl_e2^T per Hschur block
//                    (pairs from the per-phase k_ba_pair_table) and of sum_e cf_e per pose
//   k_ba_schur_fin   S block (c1,c2) = [c1==c2](Hpp+lambda I) - pair sum; bschur = bp - sum cf
//   k_ba_ldlt*       dense LDLT of the reduced camera system and the solve: 8-wide panels
//                    (k_ba_ldlt_pan), column steps (k_ba_ldlt_col) or 16-wide blocked MFMA
//                    (k_ba_ldlt), picked by size (LdltPlan)
//   k_ba_update      x_l = Dinv (bl - sum_e Hpl_e^T x_p), X += x_l; T = exp(x_p) T; scale terms
//   k_ba_errors      new chi (block partials), then
//   k_ba_lm_control  the LM verdict: partials summed by fixed_sum_wave (lane l adds partials
//                    l, l+64, ... in index order, then a butterfly over the lanes: a fixed tree,
//                    not the index-order sum of the reported chi2), accept/reject, lambda/ni,
//                    trial budget, _nBad, stop flag polled through host-mapped memory; gates
//                    the next trial's kernels.  (k_ba_errors_ctl, a debug option, does both in
//                    one launch: the verdict runs in the launch's last block.)
// In the device-LM loop k_ba_lin_schur stands for k_ba_linearize + k_ba_point_sum +
// k_ba_point_schur where the edges arrive grouped by point, and k_ba_pairs / k_ba_schur_fin take
// k_ba_cam_sum / k_ba_cam_fin's sums (BaDev::fused, camfold).
// Every reduction has a fixed partition and order: results are run-to-run
// identical.  No cross-block synchronisation in the default path; k_ba_errors_ctl's one hand-off
// is write-through partials and a release ticket with one acquire fence in the last block (an
// agent-scope release/acquire per block costs an L2 writeback/invalidate on the multi-XCD part).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <vector>

#include "ba_host.h"

namespace orbx {

// Problem intake: validation, the phase-1 sizes, one pinned-arena upload of
// the raw arrays and k_ba_prep (src/Optimizer.cc:603-745's graph assembly).
// kn: the robust kernels the edges start with (LocalBundleAdjustment's by default).
struct BaKernels {
  float th_mono, th_stereo;  // Huber deltas as the reference stores them (float)
  bool robust;
};
static const BaKernels kLocalBaKernels = {std::sqrt(5.991f), std::sqrt(7.815f), true};  // src/Optimizer.cc:653-654
orbx_status ba_intake(LocalBA& L, const orbx_ba_problem* pb, hipStream_t st, const BaKernels& kn = kLocalBaKernels) {
  L.trials = 0;
  for (double& t : L.t_struct) t = 0;
  BaDev& D = L.D;
  // test hooks (off unless orbx_debug_ba_options set them): a NaN trial, a device-raised stop flag
  D.nan_trial = ba_opts().nan_trial;
  D.raise_after = ba_opts().raise_stop_after;
  Ctx& c = L.c;
  const int nc = pb->n_cams, np = pb->n_points, ne = pb->n_edges;
  D.nc = nc;
  D.np = np;
  D.ne = ne;
  // Index checks, point order and point count in one branch-free (vectorisable) pass; the camera
  // histogram in four interleaved counter sets (a run of one camera's edges does not serialise on one
  // counter).  The host pass sits on the call's critical path: the device waits for its upload.
  const int* ep = pb->edge_point;
  const int* ec = pb->edge_cam;
  int pmin = ne > 0 ? ep[0] : 0, pmax = pmin, cmin = ne > 0 ? ec[0] : 0, cmax = cmin, ord = 1, npts = ne > 0;
  for (int e = 1; e < ne; e++) {
    const int p = ep[e], q = ep[e - 1], c = ec[e];
    pmin = std::min(pmin, p);
    pmax = std::max(pmax, p);
    cmin = std::min(cmin, c);
    cmax = std::max(cmax, c);
    ord &= p >= q;
    npts += p != q;
  }
  if (ne > 0 && (pmin < 0 || pmax >= np || cmin < 0 || cmax >= nc)) return ORBX_ERR_ARG;
  const bool grouped = ord != 0;  // edges ordered by point (the reference adds them per MapPoint)
  // grouped: some point has more than kFuseMaxDeg positions <=> ep[e] == ep[e - kFuseMaxDeg] somewhere
  int long_run = 0;
  if (grouped)
    for (int e = kFuseMaxDeg; e < ne; e++) long_run |= ep[e] == ep[e - kFuseMaxDeg];
  L.ccnt.assign(nc, 0);
  L.ccnt4.assign(4 * (size_t)nc, 0);
  int* h = L.ccnt4.data();
  int e4 = 0;
  for (; e4 + 4 <= ne; e4 += 4) {
    h[ec[e4]]++;
    h[nc + ec[e4 + 1]]++;
    h[2 * nc + ec[e4 + 2]]++;
    h[3 * nc + ec[e4 + 3]]++;
  }
  for (; e4 < ne; e4++) h[ec[e4]]++;
  for (int i = 0; i < nc; i++) L.ccnt[i] = h[i] + h[nc + i] + h[2 * nc + i] + h[3 * nc + i];
  // the fused point side needs every point's positions inside one block (else the three kernels)
  L.fuse_ok = grouped && !long_run;
  // the structure on the device when the edges arrive grouped by point (else the host build)
  L.dev_struct = grouped && nc <= kStructMaxNc && (ne + kTileE - 1) / kTileE <= kStructMaxTiles;
  if (L.dev_struct) {  // phase-1 sizes: the launches need no readback
    int nposes = 0, maxc = 0;
    for (int i = 0; i < nc; i++)
      if (L.ccnt[i] && !(pb->fixed && pb->fixed[i])) {
        nposes++;
        maxc = std::max(maxc, L.ccnt[i]);
      }
    long long nslots = 0;  // 64-bit: edges x poses
    for (int i = 0, j = 0; i < nc; i++)
      if (L.ccnt[i] && !(pb->fixed && pb->fixed[i])) nslots += (long long)L.ccnt[i] * (nposes - j++);
    // (beyond the int range: finish_structure refuses the problem)
    const int s1[5] = {ne, npts, nposes, maxc, nslots > std::numeric_limits<int>::max() ? -1 : (int)nslots};
    std::memcpy(L.sizes1, s1, sizeof s1);
  }
  if (!L.dev_struct) {  // the host structure build reads them
    L.e_pt.assign(pb->edge_point, pb->edge_point + ne);
    L.e_cam.assign(pb->edge_cam, pb->edge_cam + ne);
  }
  L.fixed.assign(nc, 0);
  Arena& A = L.prob_arena;
  if (A.reserve(arena_bytes({32 * (size_t)nc, 24 * (size_t)nc, 40 * (size_t)nc, 12 * (size_t)np, 4 * (size_t)ne,
                             4 * (size_t)ne, 12 * (size_t)ne, 4 * (size_t)ne, (size_t)nc})) != hipSuccess)
    return ORBX_ERR_HIP;
  double* cq = A.take<double>(4 * (size_t)nc);
  double* ct = A.take<double>(3 * (size_t)nc);
  double* intr = A.take<double>(5 * (size_t)nc);
  float* Xf = A.take<float>(3 * (size_t)np);
  int* ept = A.take<int>(ne);
  int* ecam = A.take<int>(ne);
  float* obs_f = A.take<float>(3 * (size_t)ne);
  float* isig_f = A.take<float>(ne);
  uint8_t* dfix = A.take<uint8_t>(nc);
  L.dfix = dfix;
  // device-only FP64 / flag arrays, filled by k_ba_prep
  const size_t al = 256;
  auto rnd = [&](size_t b) { return (std::max<size_t>(b, 1) + al - 1) / al * al; };
  const size_t o_X = 0, o_eobs = o_X + rnd(24 * (size_t)np), o_einfo = o_eobs + rnd(24 * (size_t)ne),
               o_edelta = o_einfo + rnd(8 * (size_t)ne), o_edsqr = o_edelta + rnd(8 * (size_t)ne),
               o_est = o_edsqr + rnd(4 * (size_t)ne), o_erob = o_est + rnd(ne), o_end = o_erob + rnd(ne);
  BA_CHECK(c.prob.ensure(o_end));
  double* X = reinterpret_cast<double*>(c.prob.p + o_X);
  double* eobs = reinterpret_cast<double*>(c.prob.p + o_eobs);
  double* einfo = reinterpret_cast<double*>(c.prob.p + o_einfo);
  double* edelta = reinterpret_cast<double*>(c.prob.p + o_edelta);
  float* edsqr = reinterpret_cast<float*>(c.prob.p + o_edsqr);
  uint8_t* est = c.prob.p + o_est;
  uint8_t* erob = c.prob.p + o_erob;
  // vertices: Converter::toSE3Quat (float -> double, Quaterniond(R), normalize)
  {
    double* hq = A.host(cq);
    double* ht = A.host(ct);
    double* hi = A.host(intr);
    for (int i = 0; i < nc; i++) {
      const float* T = pb->Tcw + 12 * i;
      const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
      Quat q = mat2q(R);
      qnormalize(q);
      hq[4 * i] = q.x;
      hq[4 * i + 1] = q.y;
      hq[4 * i + 2] = q.z;
      hq[4 * i + 3] = q.w;
      ht[3 * i] = T[3];
      ht[3 * i + 1] = T[7];
      ht[3 * i + 2] = T[11];
      for (int k = 0; k < 5; k++) hi[5 * i + k] = pb->intr[5 * i + k];
      L.fixed[i] = pb->fixed ? pb->fixed[i] : 0;
      A.host(dfix)[i] = L.fixed[i];
    }
    if (np) std::memcpy(A.host(Xf), pb->Xw, 12 * (size_t)np);
    if (ne) {
      std::memcpy(A.host(ept), pb->edge_point, 4 * (size_t)ne);
      std::memcpy(A.host(ecam), pb->edge_cam, 4 * (size_t)ne);
      std::memcpy(A.host(obs_f), pb->obs, 12 * (size_t)ne);
      std::memcpy(A.host(isig_f), pb->inv_sigma2, 4 * (size_t)ne);
    }
  }
  BA_CHECK(A.upload(st));
  BA_CHECK(c.cbak.ensure(7 * (size_t)nc));
  BA_CHECK(c.Xbak.ensure(3 * (size_t)np));
  BA_CHECK(c.eerr.ensure(3 * (size_t)ne));
  {
    const float thMono = kn.th_mono, thStereo = kn.th_stereo;
    const int gpre = (std::max(ne, 3 * np) + LBS - 1) / LBS;
    if (gpre > 0)
      hipLaunchKernelGGL(k_ba_prep, dim3(gpre), dim3(LBS), 0, st, ne, np, obs_f, isig_f, Xf, X, est, eobs, einfo,
                         edelta, edsqr, erob, c.eerr.p, thMono, thStereo);
    BA_CHECK(hipGetLastError());
    if (!kn.robust && ne > 0) BA_CHECK(hipMemsetAsync(erob, 0, ne, st));  // no edge carries a kernel
  }
  BA_CHECK(c.flag.ensure(ne));
  BA_CHECK(c.scal.ensure(8));
  D.cq = cq;
  D.ct = ct;
  D.cbak = c.cbak.p;
  D.intr = intr;
  D.X = X;
  D.Xbak = c.Xbak.p;
  D.ept = ept;
  D.ecam = ecam;
  D.est = est;
  D.eobs = eobs;
  D.einfo = einfo;
  D.edelta = edelta;
  D.edsqr = edsqr;
  D.erobust = erob;
  D.eerr = c.eerr.p;
  D.scal = c.scal.p;
  return ORBX_OK;
}

// Write-back (src/Optimizer.cc:817-885): the erase list, poses and points, issued on st into the
// write-back arena; the caller syncs st, then ba_writeback_finish fills its arrays.
// erase_list false (GlobalBundleAdjustemnt): no vToErase, res->edge_outlier is not touched.
orbx_status ba_writeback(LocalBA& L, const orbx_ba_problem* pb, orbx_ba_result* res, bool ran, hipStream_t st,
                         bool erase_list = true) {
  BaDev& D = L.D;
  const int nc = pb->n_cams, np = pb->n_points, ne = pb->n_edges;
  const int ge = (ne + LBS - 1) / LBS;
  res->trials = L.trials;
  res->ran = ran ? 1 : 0;
  if (!ran) {  // src/Optimizer.cc:749-751: return before any write-back
    std::memcpy(res->Tcw, pb->Tcw, sizeof(float) * 12 * nc);
    std::memcpy(res->Xw, pb->Xw, sizeof(float) * 3 * np);
    if (ne > 0) std::memset(res->edge_outlier, 0, ne);
    if (res->Tcw_d)
      for (int i = 0; i < 12 * nc; i++) res->Tcw_d[i] = pb->Tcw[i];
    if (res->Xw_d)
      for (int i = 0; i < 3 * np; i++) res->Xw_d[i] = pb->Xw[i];
    return ORBX_OK;
  }
  // :817-847 vToErase, then the poses and points; everything lands in the mapped write-back arena
  // (ba_writeback_finish moves it into the caller's arrays after the sync)
  Arena& A = L.wb_arena;
  BA_CHECK(A.reserve(arena_bytes({res->Tcw_d ? 12 * sizeof(double) * nc : 0, res->Xw_d ? 3 * sizeof(double) * np : 0,
                                  12 * sizeof(float) * nc, 3 * sizeof(float) * np, (size_t)ne})));
  LocalBA::Wb& w = L.wb;
  w.Tcw_d = res->Tcw_d ? A.take<double>(12 * (size_t)nc) : nullptr;
  w.Xw_d = res->Xw_d ? A.take<double>(3 * (size_t)np) : nullptr;
  w.Tcw = A.take<float>(12 * (size_t)nc);
  w.Xw = A.take<float>(3 * (size_t)np);
  w.flag = A.take<uint8_t>((size_t)ne);
  if (ne > 0 && erase_list) hipLaunchKernelGGL(k_ba_outliers, dim3(ge), dim3(LBS), 0, st, D, w.flag, 0);
  const int gx = (std::max(nc, np) + LBS - 1) / LBS;
  hipLaunchKernelGGL(k_ba_export, dim3(std::max(gx, 1)), dim3(LBS), 0, st, D, w.Tcw, w.Xw, w.Tcw_d, w.Xw_d);
  BA_CHECK(hipGetLastError());
  return ORBX_OK;
}

// After the stream has synchronised: the write-back arena's pinned copy into the caller's arrays.
void ba_writeback_finish(LocalBA& L, const orbx_ba_problem* pb, orbx_ba_result* res, bool ran, bool erase_list = true) {
  if (!ran) return;
  const int nc = pb->n_cams, np = pb->n_points, ne = pb->n_edges;
  Arena& A = L.wb_arena;
  const LocalBA::Wb& w = L.wb;
  if (ne > 0 && erase_list) std::memcpy(res->edge_outlier, A.host(w.flag), ne);
  std::memcpy(res->Tcw, A.host(w.Tcw), 12 * sizeof(float) * nc);
  std::memcpy(res->Xw, A.host(w.Xw), 3 * sizeof(float) * np);
  if (res->Tcw_d) std::memcpy(res->Tcw_d, A.host(w.Tcw_d), 12 * sizeof(double) * nc);
  if (res->Xw_d) std::memcpy(res->Xw_d, A.host(w.Xw_d), 3 * sizeof(double) * np);
}

orbx_status run_local_ba(LocalBA& L, const orbx_ba_problem* pb, orbx_ba_result* res, const StopFlag& stop,
                         hipStream_t st) {
  double host_build_ms = 0;
  const auto t_start = std::chrono::steady_clock::now();
  // host-side marks for the trace line: intake, phase-1 structure, phase 1, phase-2 structure, phase 2
  std::chrono::steady_clock::time_point tm[5];
  for (auto& t : tm) t = t_start;
  orbx_status s0 = ba_intake(L, pb, st);
  if (s0 != ORBX_OK) return s0;
  tm[0] = std::chrono::steady_clock::now();
  BaDev& D = L.D;
  Ctx& c = L.c;
  const int ne = pb->n_edges;
  res->iterations[0] = res->iterations[1] = 0;
  res->trials = 0;
  res->chi2[0] = res->chi2[1] = 0;
  const int ge = (ne + LBS - 1) / LBS;
  bool ran = false;
  // LM control on the device; the stop flag it polls lives in pinned, device-mapped memory
  DevStop dstop{nullptr, nullptr};
  L.unmap_stop();
  L.hook_stopped = false;
  if (!L.map_stop(stop, &dstop)) return ORBX_ERR_HIP;
  auto optimize = [&](int iterations, int* iters, double* chi, const std::function<hipError_t()>& spec = nullptr) {
    return L.optimize_dev(iterations, stop, dstop, st, iters, chi, spec);
  };
  // phase 2's outlier marking and structure, queued behind phase 1's readback and gated on its LM
  // state (spec_skip): when phase 1 ends on an accepted state the one readback also brings phase
  // 2's sizes, so the call pays one host round trip between the phases instead of two
  const bool spec2 = L.dev_struct && ne > 0;
  BaDev Dspec = D;  // (filled below, after the phase-1 structure)
  auto spec = [&]() -> hipError_t {
    // the gate is read here, not when Dspec is filled: optimize_dev allocates the LM state on a
    // handle's first call, after the phase-1 structure (an ungated launch would run mid-phase)
    if (!c.lm.p) return hipErrorInvalidValue;
    Dspec.lm = c.lm.p;
    hipLaunchKernelGGL(k_ba_outliers, dim3(ge), dim3(LBS), 0, st, Dspec, c.flag.p, 1);
    HIP_TRY(hipGetLastError());
    return L.launch_structure_dev(0, st, nullptr, c.lm.p);
  };
  if (!(stop())) {  // src/Optimizer.cc:749-751
    ran = true;
    if (!L.dev_struct) L.level.assign(ne, 0);
    const auto tb0 = std::chrono::steady_clock::now();
    orbx_status s = L.build_structure(-1, st);
    const auto tb1 = std::chrono::steady_clock::now();
    host_build_ms += std::chrono::duration<double, std::milli>(tb1 - tb0).count();
    tm[1] = tb1;
    if (s != ORBX_OK) return s;
    Dspec = D;
    L.cap.cur_phase = 0;
    s = optimize(5, &res->iterations[0], &res->chi2[0], spec2 ? std::function<hipError_t()>(spec) : nullptr);
    if (s != ORBX_OK) return s;
    // did the speculative phase-2 launches run (spec_skip's condition: phase 1 ended done, nothing to
    // pop or refresh, and not on the stop flag)?
    const bool spec_ran =
        spec2 && L.lm_host()->done && !L.lm_host()->refresh && !L.lm_host()->rejected && !L.lm_host()->stopped;
    tm[2] = tm[3] = tm[4] = std::chrono::steady_clock::now();
    if (!(stop()) && !L.hook_stopped) {
      // :764-802 level-1 outliers, drop robust kernels (already done on the device when spec_ran)
      if (ne > 0 && !spec_ran) hipLaunchKernelGGL(k_ba_outliers, dim3(ge), dim3(LBS), 0, st, D, c.flag.p, 1);
      BA_CHECK(hipGetLastError());
      if (!L.dev_struct) {
        BA_CHECK(hipMemcpyAsync(L.level.data(), c.flag.p, ne, hipMemcpyDeviceToHost, st));
        BA_CHECK(hipStreamSynchronize(st));
      }
      const auto tb2 = std::chrono::steady_clock::now();
      if (spec_ran) {
        const int* sz = L.sint.as<int>();  // written by the speculative k_ba_struct_scan before the readback's event
        s = L.finish_structure(sz[0], sz[1], sz[2], sz[3], sz[4], st);
      } else {
        s = L.build_structure(0, st);
      }
      tm[3] = std::chrono::steady_clock::now();
      host_build_ms += std::chrono::duration<double, std::milli>(tm[3] - tb2).count();
      if (s != ORBX_OK) return s;
      L.cap.cur_phase = 1;
      s = optimize(10, &res->iterations[1], &res->chi2[1]);
      if (s != ORBX_OK) return s;
      tm[4] = std::chrono::steady_clock::now();
    }
  }
  BA_CHECK(ba_writeback(L, pb, res, ran, st));
  L.unmap_stop();
  if (!ran) return ORBX_OK;
  BA_CHECK(hipStreamSynchronize(st));
  ba_writeback_finish(L, pb, res, ran);
  if (ba_opts().trace) {
    const auto t_end = std::chrono::steady_clock::now();
    auto d = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
      return std::chrono::duration<double, std::milli>(b - a).count();
    };
    std::fprintf(stderr,
                 "[orbx_ba] total %.3f ms, structure %.3f ms (host index %.3f, host poses %.3f, device %.3f, upload %.3f), "
                 "iterations %d+%d, trials %d; host marks: intake %.3f, struct1 %.3f, phase1 %.3f, struct2 %.3f, "
                 "phase2 %.3f, writeback %.3f ms\n",
                 d(t_start, t_end), host_build_ms, L.t_struct[0], L.t_struct[1], L.t_struct[2], L.t_struct[3],
                 res->iterations[0], res->iterations[1], res->trials, d(t_start, tm[0]), d(tm[0], tm[1]),
                 d(tm[1], tm[2]), d(tm[2], tm[3]), d(tm[3], tm[4]), d(tm[4], t_end));
  }
  return ORBX_OK;
}

}  // namespace orbx
#include "ba_global.h"  // run_global_ba: Optimizer::GlobalBundleAdjustemnt on the parts above
namespace orbx {

// ---- batched driver: K independent problems through the same launches ----
// Every trial kernel runs once for all K problems (blockIdx.z), each block on
// its own problem's arrays and LM state; grids span the largest problem and
// the smaller ones' extra blocks return at once.  Per problem the arithmetic,
// partitions and reduction orders are those of the single-problem device LM
// loop, so every problem's result is bit-identical to running it alone.
struct BaBatch {
  DevBuf<BaDev> dev;       // [Dg_0..Dg_K-1, D0_0..D0_K-1]
  DevBuf<LmState> lm;      // K
  PinnedBuf lm_pin;
  LmState* lm_host() const { return lm_pin.as<LmState>(); }  // K states
  std::vector<BaDev> hostD;
};

orbx_status optimize_many(LocalBA* const* Ls, int K, BaBatch& B, int iterations, const StopFlag& stop,
                          const DevStop& dstop, hipStream_t st, int* iters, double* chis) {
  int Nmax = 0, gaM = 1, gpM = 1, geM = 1, gnpM = 1, nbpM = 0, gsM = 1, nposM = 0, nbfM = 0, n_unfused = 0;
  for (int i = 0; i < K; i++) {
    const BaDev& D = Ls[i]->D;
    nbfM = std::max(nbfM, D.nbf);
    n_unfused += D.nbf > 0 ? 0 : 1;
    Nmax = std::max(Nmax, 6 * D.nposes);
    gaM = std::max(gaM, (D.na + LBS - 1) / LBS);
    gpM = std::max(gpM, D.nbu);
    geM = std::max(geM, D.nbe);
    gnpM = std::max(gnpM, (D.npa + LBS - 1) / LBS);
    nbpM = std::max(nbpM, D.nblk + D.nposes);
    gsM = std::max(gsM, D.gsplit);
    nposM = std::max(nposM, D.nposes);
  }
  // each problem takes the LDLT kernel a single call would (bit-identical results): the panel
  // kernel for the small systems, the column-step one (or the MFMA-blocked opt-in) for the rest
  int Npan = 0, Ncol = 0;
  for (int i = 0; i < K; i++) {
    const int Ni = 6 * Ls[i]->D.nposes;
    if (ldlt_use_pan(Ni)) Npan = std::max(Npan, Ni); else Ncol = std::max(Ncol, Ni);
  }
  LdltPlan ldlt, lpan;
  if (Ncol > 0 || Npan == 0) {
    BA_CHECK(ldlt.prepare(std::max(Ncol, 6), false));
    if (!ldlt.col) return ORBX_ERR_SIZE;  // the caller runs the problems one by one
    BA_CHECK(ldlt.prepare_many());
  }
  if (Npan > 0) {
    BA_CHECK(lpan.prepare(Npan));
    if (!lpan.pan) return ORBX_ERR_SIZE;
    BA_CHECK(lpan.prepare_many());
  }
  const bool camfold = true;
  int n_ps = 0, n_psfold = 0;  // problems that launch k_ba_point_schur / whose k_ba_lin_schur takes it
  BA_CHECK(B.lm_pin.ensure(sizeof(LmState) * K));
  BA_CHECK(B.lm.ensure(K));
  BA_CHECK(B.dev.ensure(2 * (size_t)K));
  B.hostD.resize(2 * (size_t)K);
  for (int i = 0; i < K; i++) {
    B.hostD[i] = Ls[i]->D;
    B.hostD[i].lm = B.lm.p + i;
    B.hostD[i].fused = fused_mode(B.hostD[i].nbf, B.hostD[i].nposes);
    n_ps += B.hostD[i].fused == 2 ? 0 : 1;
    n_psfold += B.hostD[i].fused == 2 ? 1 : 0;
    B.hostD[i].camfold = camfold ? 1 : 0;
    set_trial_folds(B.hostD[i]);
    B.hostD[i].ldlt_pan = ldlt_use_pan(6 * B.hostD[i].nposes) ? 1 : 0;
    B.hostD[K + i] = Ls[i]->D;
    B.hostD[K + i].lm = nullptr;
  }
  BA_CHECK(hipMemcpyAsync(B.dev.p, B.hostD.data(), sizeof(BaDev) * 2 * K, hipMemcpyHostToDevice, st));
  const BaDev* Dg = B.dev.p;
  const BaDev* D0 = B.dev.p + K;
  if (nbfM > 0)
    BA_CHECK(set_smem_attr((const void*)k_ba_lin_schur_many, kFuseSmem));
  // the entry launches (D0: no LM state, nothing fused) and the gated trials: per problem either
  // k_ba_lin_schur or the three separate kernels do the point side (each returns for the other)
  auto linearize = [&](const BaDev* Ds) {
    const bool gated = Ds == Dg;
    if (gated && nbfM > 0) hipLaunchKernelGGL(k_ba_lin_schur_many, dim3(nbfM, 1, K), dim3(kFuseNT), kFuseSmem, st, Ds);
    if (!gated || n_unfused > 0) {
      hipLaunchKernelGGL(k_ba_linearize_many, dim3(gaM, 1, K), dim3(LBS), 0, st, Ds);
      hipLaunchKernelGGL(k_ba_point_sum_many, dim3(gnpM, 1, K), dim3(LBS), 0, st, Ds);
    }
    if (nposM > 0 && !(gated && camfold)) {
      hipLaunchKernelGGL(k_ba_cam_sum_many, dim3(nposM, gsM, K), dim3(kGB), 0, st, Ds);
      hipLaunchKernelGGL(k_ba_cam_fin_many, dim3(nposM, 1, K), dim3(64), 0, st, Ds);
    }
  };
  for (int i = 0; i < K; i++) iters[i] = 0;
  if (!(stop())) {
    hipLaunchKernelGGL(k_ba_errors_many, dim3(geM, 1, K), dim3(LBS), 0, st, D0, 1, 0);
    linearize(D0);
    hipLaunchKernelGGL(k_ba_dmax_many, dim3(1, 1, K), dim3(1024), 0, st, D0);
    hipLaunchKernelGGL(k_ba_lm_init_many, dim3(1, 1, K), dim3(64), 0, st, Dg, iterations);
    BA_CHECK(hipGetLastError());
    for (int budget = iterations, first = 1;; first = 0) {
      for (int t = 0; t < budget; t++) {
        if (!(first && t == 0))
          linearize(Dg);  // gated per problem
        else if (n_psfold > 0)
          hipLaunchKernelGGL(k_ba_lin_schur_many, dim3(nbfM, 1, K), dim3(kFuseNT), kFuseSmem, st, Dg);
        if (n_ps > 0) hipLaunchKernelGGL(k_ba_point_schur_many, dim3(gaM, 1, K), dim3(LBS), 0, st, Dg, 0.0);
        if (nposM > 0) {
          hipLaunchKernelGGL(k_ba_pairs_many, dim3(nbpM, gsM, K), dim3(kPB), 0, st, Dg);
          hipLaunchKernelGGL(k_ba_schur_fin_many, dim3(nbpM, 1, K), dim3(64), 0, st, Dg, 0.0);
          if (Npan > 0) lpan.launch_many(Dg, K, st);
          if (Ncol > 0) ldlt.launch_many(Dg, K, st);
        }
        hipLaunchKernelGGL(k_ba_update_many, dim3(gpM, 1, K), dim3(LBS), 0, st, Dg, 0.0);
        hipLaunchKernelGGL(k_ba_errors_many, dim3(geM, 1, K), dim3(LBS), 0, st, Dg, 1, 1);
        hipLaunchKernelGGL(k_ba_lm_control_many, dim3(1, 1, K), dim3(64), 0, st, Dg, dstop);
      }
      hipLaunchKernelGGL(k_ba_errors_many, dim3(geM, 1, K), dim3(LBS), 0, st, D0, 0, 0);
      hipLaunchKernelGGL(k_ba_lm_final_many, dim3(1, 1, K), dim3(64), 0, st, Dg);
      BA_CHECK(hipGetLastError());
      BA_CHECK(hipMemcpyAsync(B.lm_host(), B.lm.p, sizeof(LmState) * K, hipMemcpyDeviceToHost, st));
      BA_CHECK(hipEventRecord(Ls[0]->rb_ev, st));
      BA_CHECK(Ls[0]->wait_event(Ls[0]->rb_ev));  // keeps the device's stop mirror current
      int left = 0;
      bool refresh = false;
      for (int i = 0; i < K; i++) {
        if (!B.lm_host()[i].done || B.lm_host()[i].refresh) left = std::max(left, iterations - B.lm_host()[i].it);
        refresh |= B.lm_host()[i].refresh != 0;
      }
      if (left == 0) break;
      if (refresh) {  // problems paused on a NaN-rho rejection (all three launches gated per problem)
        hipLaunchKernelGGL(k_ba_restore_many, dim3(gpM, 1, K), dim3(LBS), 0, st, Dg);
        hipLaunchKernelGGL(k_ba_errors_many, dim3(geM, 1, K), dim3(LBS), 0, st, Dg, 2, 0);
        hipLaunchKernelGGL(k_ba_lm_resume_many, dim3(1, 1, K), dim3(64), 0, st, Dg);
        BA_CHECK(hipGetLastError());
      }
      budget = std::max(1, left);
    }
    bool rej = false;
    for (int i = 0; i < K; i++) {
      iters[i] = B.lm_host()[i].it;
      Ls[i]->trials += B.lm_host()[i].trials;
      chis[i] = B.lm_host()[i].final_chi;
      rej |= B.lm_host()[i].rejected != 0;
    }
    if (rej) {  // the pops of problems that ended on a rejected trial (gated per problem)
      hipLaunchKernelGGL(k_ba_restore_many, dim3(gpM, 1, K), dim3(LBS), 0, st, Dg);
      BA_CHECK(hipGetLastError());
    }
  } else {
    hipLaunchKernelGGL(k_ba_errors_many, dim3(geM, 1, K), dim3(LBS), 0, st, D0, 0, 0);
    hipLaunchKernelGGL(k_ba_lm_final_many, dim3(1, 1, K), dim3(64), 0, st, Dg);
    BA_CHECK(hipGetLastError());
    BA_CHECK(hipMemcpyAsync(B.lm_host(), B.lm.p, sizeof(LmState) * K, hipMemcpyDeviceToHost, st));
    BA_CHECK(hipStreamSynchronize(st));
    for (int i = 0; i < K; i++) chis[i] = B.lm_host()[i].final_chi;
  }
  return ORBX_OK;
}

// K LocalBundleAdjustment calls at once: per-problem intake and structure,
// each LM phase batched, per-problem write-back.  Problems that need the host
// structure build or a reduced system beyond the column-step kernel run one
// by one instead (same results).
orbx_status run_local_ba_many(LocalBA* const* Ls, int K, BaBatch& B, const orbx_ba_problem* pbs,
                              orbx_ba_result* ress, const StopFlag& stop, hipStream_t st) {
  for (int i = 0; i < K; i++) {
    orbx_status s = ba_intake(*Ls[i], &pbs[i], st);
    if (s != ORBX_OK) return s;
  }
  DevStop dstop{nullptr, nullptr};
  for (int i = 0; i < K; i++) Ls[i]->unmap_stop();
  if (!Ls[0]->map_stop(stop, &dstop)) return ORBX_ERR_HIP;
  bool batch = true;
  for (int i = 0; i < K; i++) batch &= Ls[i]->dev_struct;
  if (!batch) {  // one by one (intake again inside: the arenas are reused)
    for (int i = 0; i < K; i++) {
      orbx_status s = run_local_ba(*Ls[i], &pbs[i], &ress[i], stop, st);
      if (s != ORBX_OK) return s;
    }
    return ORBX_OK;
  }
  std::vector<int> it(K);
  std::vector<double> chi(K);
  for (int i = 0; i < K; i++) {
    ress[i].iterations[0] = ress[i].iterations[1] = 0;
    ress[i].trials = 0;
    ress[i].chi2[0] = ress[i].chi2[1] = 0;
  }
  bool ran = false;
  if (!(stop())) {  // src/Optimizer.cc:749-751
    ran = true;
    for (int i = 0; i < K; i++) BA_CHECK(Ls[i]->build_structure(-1, st));
    orbx_status s = optimize_many(Ls, K, B, 5, stop, dstop, st, it.data(), chi.data());
    if (s == ORBX_ERR_SIZE) {  // reduced system beyond the column-step kernel: one by one
      for (int i = 0; i < K; i++) {
        s = run_local_ba(*Ls[i], &pbs[i], &ress[i], stop, st);
        if (s != ORBX_OK) return s;
      }
      return ORBX_OK;
    }
    if (s != ORBX_OK) return s;
    bool hook = false;
    for (int i = 0; i < K; i++) {
      ress[i].iterations[0] = it[i];
      ress[i].chi2[0] = chi[i];
      hook |= B.lm_host()[i].stopped && Ls[i]->D.raise_after >= 0;
    }
    if (!(stop()) && !hook) {
      for (int i = 0; i < K; i++) {  // :764-802 level-1 outliers, drop robust kernels
        const int ne = pbs[i].n_edges;
        if (ne > 0)
          hipLaunchKernelGGL(k_ba_outliers, dim3((ne + LBS - 1) / LBS), dim3(LBS), 0, st, Ls[i]->D, Ls[i]->c.flag.p, 1);
        BA_CHECK(hipGetLastError());
      }
      for (int i = 0; i < K; i++) BA_CHECK(Ls[i]->build_structure(0, st));
      s = optimize_many(Ls, K, B, 10, stop, dstop, st, it.data(), chi.data());
      if (s != ORBX_OK) return s;
      for (int i = 0; i < K; i++) {
        ress[i].iterations[1] = it[i];
        ress[i].chi2[1] = chi[i];
      }
    }
  }
  for (int i = 0; i < K; i++) BA_CHECK(ba_writeback(*Ls[i], &pbs[i], &ress[i], ran, st));
  Ls[0]->unmap_stop();
  BA_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < K; i++) ba_writeback_finish(*Ls[i], &pbs[i], &ress[i], ran);
  return ORBX_OK;
}

}  // namespace orbx

struct orbx_ba {
  int device = 0;
  hipStream_t st = nullptr;
  orbx_ba_debug_options opts = orbx::kBaOptsDefault;
  orbx::LocalBA L;
  std::vector<std::unique_ptr<orbx::LocalBA>> more;  // orbx_ba_run_many: problems 1..K-1
  orbx::BaBatch batch;
};

// A problem / result pair of orbx_ba_run, orbx_ba_run_bool and orbx_ba_run_many: sizes not negative,
// and every array a non-zero size asks for is given.
static bool valid_call(const orbx_ba_problem* p, const orbx_ba_result* r) {
  if (p->n_cams < 0 || p->n_points < 0 || p->n_edges < 0) return false;
  if (p->n_cams > 0 && (!p->Tcw || !p->intr || !r->Tcw)) return false;
  if (p->n_points > 0 && (!p->Xw || !r->Xw)) return false;
  if (p->n_edges > 0 && (!p->edge_point || !p->edge_cam || !p->obs || !p->inv_sigma2 || !r->edge_outlier))
    return false;
  return true;
}

extern "C" {

orbx_status orbx_ba_create_priority(int device, int priority, orbx_ba** out) {
  if (!out) return ORBX_ERR_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ORBX_ERR_NODEV;
  if (device < 0 || device >= n) return ORBX_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return ORBX_ERR_HIP;
  orbx_ba* h = new (std::nothrow) orbx_ba();
  if (!h) return ORBX_ERR_HIP;
  h->device = device;
  hipError_t e;
  if (priority == 0) {
    e = hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking);
  } else {
    int least = 0, greatest = 0;
    e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e == hipSuccess) {
      const int p = std::min(std::max(priority, std::min(least, greatest)), std::max(least, greatest));
      e = hipStreamCreateWithPriority(&h->st, hipStreamNonBlocking, p);
    }
  }
  if (e != hipSuccess) {
    delete h;
    return ORBX_ERR_HIP;
  }
  *out = h;
  return ORBX_OK;
}

orbx_status orbx_ba_create(int device, orbx_ba** out) { return orbx_ba_create_priority(device, 0, out); }

orbx_status orbx_stream_create(int device, const uint32_t* cu_mask, int cu_mask_words, void** stream) {
  if (!stream || cu_mask_words < 0 || (cu_mask_words > 0 && !cu_mask)) return ORBX_ERR_ARG;
  *stream = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ORBX_ERR_NODEV;
  if (device < 0 || device >= n) return ORBX_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return ORBX_ERR_HIP;
  hipStream_t st = nullptr;
  const hipError_t e = cu_mask_words > 0 ? hipExtStreamCreateWithCUMask(&st, (uint32_t)cu_mask_words, cu_mask)
                                         : hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  if (e != hipSuccess) return ORBX_ERR_HIP;
  *stream = (void*)st;
  return ORBX_OK;
}

void orbx_stream_destroy(void* stream) {
  if (!stream) return;
  (void)hipStreamSynchronize((hipStream_t)stream);
  (void)hipStreamDestroy((hipStream_t)stream);
}

orbx_status orbx_ba_create_masked(int device, const uint32_t* cu_mask, int cu_mask_words, orbx_ba** out) {
  if (!out) return ORBX_ERR_ARG;
  *out = nullptr;
  void* st = nullptr;
  const orbx_status s = orbx_stream_create(device, cu_mask, cu_mask_words, &st);
  if (s != ORBX_OK) return s;
  orbx_ba* h = new (std::nothrow) orbx_ba();
  if (!h) {
    orbx_stream_destroy(st);
    return ORBX_ERR_HIP;
  }
  h->device = device;
  h->st = (hipStream_t)st;
  *out = h;
  return ORBX_OK;
}

orbx_status orbx_ba_run_many(orbx_ba* h, int n, const orbx_ba_problem* problems, orbx_ba_result* results,
                             const volatile int* stop_flag) {
  if (!h || n < 0 || (n > 0 && (!problems || !results))) return ORBX_ERR_ARG;
  if (n == 0) return ORBX_OK;
  for (int i = 0; i < n; i++)
    if (!valid_call(&problems[i], &results[i])) return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  while ((int)h->more.size() < n - 1) {
    h->more.emplace_back(new (std::nothrow) orbx::LocalBA());
    if (!h->more.back()) {
      h->more.pop_back();
      return ORBX_ERR_HIP;
    }
  }
  std::vector<orbx::LocalBA*> Ls(n);
  Ls[0] = &h->L;
  for (int i = 1; i < n; i++) Ls[i] = h->more[i - 1].get();
  h->L.cap.sel_phase = -1;  // (the batched driver does not capture)
  orbx::BaOptScope scope(&h->opts);
  orbx::StopFlag sf;
  sf.i = stop_flag;
  return orbx::run_local_ba_many(Ls.data(), n, h->batch, problems, results, sf, h->st);
}

int orbx_debug_ba_capture_select(orbx_ba* h, int phase, int it, int q) {
  if (!h || phase > 1 || (phase >= 0 && (it < -1 || q < 0))) return ORBX_ERR_ARG;
  orbx::BaCapture& c = h->L.cap;
  c.sel_phase = phase < 0 ? -1 : phase;
  c.sel_it = it;
  c.sel_q = q;
  c.have = false;
  return ORBX_OK;
}

long long orbx_debug_ba_capture_read(orbx_ba* h, int what, void* dst, size_t cap) {
  if (!h || (cap > 0 && !dst)) return ORBX_ERR_ARG;
  const orbx::BaCapture& c = h->L.cap;
  const bool fired = c.have && c.hi[0] != 0;
  const void* src = nullptr;
  size_t bytes = 0;
  int hdr[12];
  if (what == ORBX_BA_CAP_HEADER) {
    const int* d = c.dims;
    const int v[12] = {fired ? 1 : 0,        fired ? d[0] : -1,    fired ? c.hi[1] : -1, fired ? c.hi[2] : -1,
                       fired ? c.hi[3] : 0,  fired ? c.hi[5] : -1, fired ? d[1] : 0,     fired ? d[2] : 0,
                       fired ? d[3] : 0,     fired ? d[4] : 0,     fired ? d[5] : 0,     fired ? d[6] : 0};
    std::memcpy(hdr, v, sizeof v);
    src = hdr;
    bytes = sizeof hdr;
  } else {
    bool is_int;
    size_t off, cnt;
    if (!orbx::BaCapture::item(what, c.dims, &is_int, &off, &cnt)) return ORBX_ERR_ARG;
    if (!fired) return ORBX_ERR_STATE;
    src = is_int ? (const void*)(c.hi.data() + off) : (const void*)(c.hd.data() + off);
    bytes = cnt * (is_int ? sizeof(int) : sizeof(double));
  }
  if (dst && bytes) std::memcpy(dst, src, std::min(cap, bytes));
  return (long long)bytes;
}

int orbx_debug_ba_options(orbx_ba* h, const orbx_ba_debug_options* o) {
  if (!h) return ORBX_ERR_ARG;
  if (o && (o->ldlt < ORBX_BA_LDLT_AUTO || o->ldlt > ORBX_BA_LDLT_TILED)) return ORBX_ERR_ARG;
  h->opts = o ? *o : orbx::kBaOptsDefault;
  return ORBX_OK;
}

orbx_status orbx_ba_stop_flag(orbx_ba* h, volatile int** flag) {
  if (!h || !flag) return ORBX_ERR_ARG;
  if (!h->L.own_stop.p) {
    (void)hipSetDevice(h->device);
    if (h->L.own_stop.ensure(sizeof(int)) != hipSuccess) return ORBX_ERR_HIP;
    *h->L.own_stop.as<int>() = 0;
  }
  *flag = h->L.own_stop.as<int>();
  return ORBX_OK;
}

orbx_status orbx_ba_destroy(orbx_ba* h) {
  if (!h) return ORBX_ERR_ARG;
  (void)hipSetDevice(h->device);
  if (h->st) (void)hipStreamDestroy(h->st);
  delete h;
  return ORBX_OK;
}

orbx_status orbx_ba_run(orbx_ba* h, const orbx_ba_problem* p, orbx_ba_result* r, const volatile int* stop_flag) {
  if (!h || !p || !r || !valid_call(p, r)) return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  orbx::BaOptScope scope(&h->opts);
  orbx::StopFlag f;
  f.i = stop_flag;
  const orbx_status s = orbx::run_local_ba(h->L, p, r, f, h->st);
  h->L.cap.sel_phase = -1;  // a capture selection holds for one run
  return s;
}

orbx_status orbx_ba_run_bool(orbx_ba* h, const orbx_ba_problem* p, orbx_ba_result* r, const volatile bool* stop_flag) {
  if (!h || !p || !r || !valid_call(p, r)) return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  orbx::BaOptScope scope(&h->opts);
  orbx::StopFlag f;
  f.b = stop_flag;
  const orbx_status s = orbx::run_local_ba(h->L, p, r, f, h->st);
  h->L.cap.sel_phase = -1;
  return s;
}

// orbx_ba_run_global's arguments: as valid_call, but the erase list is optional (there is none)
static bool valid_global_call(const orbx_ba_problem* p, const orbx_ba_result* r) {
  if (p->n_cams < 0 || p->n_points < 0 || p->n_edges < 0) return false;
  if (p->n_cams > 0 && (!p->Tcw || !p->intr || !r->Tcw)) return false;
  if (p->n_points > 0 && (!p->Xw || !r->Xw)) return false;
  if (p->n_edges > 0 && (!p->edge_point || !p->edge_cam || !p->obs || !p->inv_sigma2)) return false;
  return true;
}

static orbx_status ba_run_global(orbx_ba* h, const orbx_ba_problem* p, int n_iterations, int robust, orbx_ba_result* r,
                                 uint8_t* point_included, const orbx::StopFlag& f) {
  if (!h || !p || !r || !valid_global_call(p, r)) return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  orbx::BaOptScope scope(&h->opts);
  const orbx_status s = orbx::run_global_ba(h->L, p, n_iterations, robust != 0, r, point_included, f, h->st);
  h->L.cap.sel_phase = -1;
  return s;
}

orbx_status orbx_ba_run_global(orbx_ba* h, const orbx_ba_problem* p, int n_iterations, int robust, orbx_ba_result* r,
                               uint8_t* point_included, const volatile int* stop_flag) {
  orbx::StopFlag f;
  f.i = stop_flag;
  return ba_run_global(h, p, n_iterations, robust, r, point_included, f);
}

orbx_status orbx_ba_run_global_bool(orbx_ba* h, const orbx_ba_problem* p, int n_iterations, int robust,
                                    orbx_ba_result* r, uint8_t* point_included, const volatile bool* stop_flag) {
  orbx::StopFlag f;
  f.b = stop_flag;
  return ba_run_global(h, p, n_iterations, robust, r, point_included, f);
}

orbx_status orbx_local_ba(const orbx_ba_problem* p, orbx_ba_result* r, const volatile int* stop_flag, int device) {
  orbx_ba* h = nullptr;
  orbx_status s = orbx_ba_create(device, &h);
  if (s != ORBX_OK) return s;
  s = orbx_ba_run(h, p, r, stop_flag);
  orbx_ba_destroy(h);
  return s;
}

}  // extern "C"

// Debug/benchmark probe (include/orbx_debug.h): solve S x = b (N = 6 * nposes)
// with the LocalBA LDLT kernel; ms = average kernel time over reps launches.
#ifdef ORBX_LS_PROBE
extern "C" int orbx_debug_ls_probe(unsigned long long* out) {  // 1024 x 8 words (probe build only)
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(orbx::g_ls_probe), sizeof(unsigned long long) * 1024 * 8) == hipSuccess ? 0 : -3;
}
#endif
extern "C" int orbx_debug_ldlt(const double* S, const double* b, int N, double* x, int reps, float* ms) {
  return orbx_debug_ldlt_ex(S, b, N, x, reps, ms, ORBX_BA_LDLT_AUTO, nullptr);
}

extern "C" int orbx_debug_ldlt_ex(const double* S, const double* b, int N, double* x, int reps, float* ms, int kind,
                                  unsigned long long* stamps) {
  if (!S || !b || !x || N <= 0 || N % 6 || reps < 1) return ORBX_ERR_ARG;
  if (kind < ORBX_BA_LDLT_AUTO || kind > ORBX_BA_LDLT_TILED) return ORBX_ERR_ARG;
  orbx_ba_debug_options o = orbx::kBaOptsDefault;
  o.ldlt = kind;
  orbx::BaOptScope scope(&o);
  const int stage_limit = 99;
  orbx::BaDev D{};
  D.nposes = N / 6;
  const size_t nn = (size_t)N * N;
  orbx::DevBuf<double> dS, dS0, db, dx, dscal, dSw;
  orbx::DevBuf<unsigned long long> ddbg;
  orbx::Event e0, e1;
  hipError_t e = dS.ensure(nn);
  if (e == hipSuccess) e = dS0.upload(S, nn);
  if (e == hipSuccess) e = db.upload(b, N);
  if (e == hipSuccess) e = dx.ensure(N);
  if (e == hipSuccess) e = dscal.ensure(8);
  D.S = dS.p;
  D.bs = db.p;
  D.xp = dx.p;
  D.scal = dscal.p;
  const bool want_ts = stamps != nullptr;
  if (e == hipSuccess && want_ts) {
    e = ddbg.ensure(64);
    if (e == hipSuccess) e = hipMemset(ddbg.p, 0, 64 * sizeof(unsigned long long));
  }
  D.dbg = ddbg.p;
  // (the single-workgroup kernels stop at a padded size of kLdltMaxNp, the tiled ones at kTiledMaxN)
  if (orbx::LdltPlan::use_tiled(N) ? N > orbx::kTiledMaxN : orbx::ldlt_np(N) > orbx::kLdltMaxNp) e = hipErrorInvalidValue;
  orbx::LdltPlan plan;
  if (e == hipSuccess) e = plan.prepare(N);
  D.ldlt_pan = plan.pan ? 1 : 0;
  if (e == hipSuccess && plan.sw_doubles() > 0) e = dSw.ensure(plan.sw_doubles());
  D.Sw = dSw.p;
  float total = 0;
  if (e == hipSuccess) e = e0.ensure(hipEventDefault);
  if (e == hipSuccess) e = e1.ensure(hipEventDefault);
  for (int r = 0; r < reps && e == hipSuccess; r++) {
    e = hipMemcpy(dS.p, dS0.p, nn * sizeof(double), hipMemcpyDeviceToDevice);
    (void)hipEventRecord(e0, nullptr);
    plan.launch(D, nullptr, stage_limit);
    (void)hipEventRecord(e1, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float t = 0;
    (void)hipEventElapsedTime(&t, e0, e1);
    total += t;
  }
  double ok = 0;
  if (e == hipSuccess) e = hipMemcpy(x, dx.p, N * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(&ok, dscal.p + 2, sizeof(double), hipMemcpyDeviceToHost);
  if (ms) *ms = total / reps;
  // the kernel's s_memtime stamps (LDLT_TS points; 0 = not reached) of the last launch
  if (ddbg.p && hipMemcpy(stamps, ddbg.p, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
    e = hipErrorUnknown;
  if (e != hipSuccess) return ORBX_ERR_HIP;
  return ok != 0.0 ? ORBX_OK : ORBX_ERR_STATE;
}

// ba_global.h -- Optimizer::GlobalBundleAdjustemnt -> Optimizer::BundleAdjustment (src/Optimizer.cc:41-284)
// on the LocalBA solver (localba.hip includes this after its own entry: ba_intake, ba_writeback and
// LocalBA::optimize_dev are the parts it shares).  The same g2o graph -- BlockSolver_6_3, the two
// projection edges, Huber kernels, Levenberg -- driven differently:
//   one optimize(nIterations) on every edge (no outlier pass, no second phase, no erase list);
//   robust kernels only with bRobust, their deltas thHuber2D = sqrt(5.99), thHuber3D = sqrt(7.815)
//   (double square roots stored in floats, :96-97; not LocalBundleAdjustment's sqrt(5.991f));
//   no early return on the stop flag: a flag raised before the call makes optimize() run zero
//   iterations (its loop head polls terminate()), and the write-back (:228-282) still happens, so
//   the outputs are then the inputs through Converter::toSE3Quat / toCvMat;
//   vbNotIncludedMP (:209-217): a point that ended with no edge is removed from the graph and
//   keeps its position.
// A global map's reduced system goes beyond the single-workgroup LDLT kernels: LdltPlan takes the
// tiled kernels (ba_ldlt.h) there, up to kTiledMaxPoses free keyframes (ORBX_ERR_SIZE beyond).
#pragma once
#include <cmath>
#include <cstring>

namespace orbx {

inline BaKernels global_ba_kernels(bool robust) {
  return BaKernels{(float)std::sqrt(5.99), (float)std::sqrt(7.815), robust};  // :96-97
}

inline orbx_status run_global_ba(LocalBA& L, const orbx_ba_problem* pb, int n_iterations, bool robust,
                                 orbx_ba_result* res, uint8_t* point_included, const StopFlag& stop, hipStream_t st) {
  const int np = pb->n_points, ne = pb->n_edges;
  orbx_status s = ba_intake(L, pb, st, global_ba_kernels(robust));
  if (s != ORBX_OK) return s;
  res->iterations[0] = res->iterations[1] = 0;
  res->trials = 0;
  res->chi2[0] = res->chi2[1] = 0;
  // :123-217 nEdges per point (the caller lists only the edges the reference adds)
  if (point_included) {
    if (np > 0) std::memset(point_included, 0, np);
    for (int e = 0; e < ne; e++) point_included[pb->edge_point[e]] = 1;
  }
  DevStop dstop{nullptr, nullptr};
  L.unmap_stop();
  L.hook_stopped = false;
  if (!L.map_stop(stop, &dstop)) return ORBX_ERR_HIP;
  if (!L.dev_struct) L.level.assign(ne, 0);
  s = L.build_structure(-1, st);  // initializeOptimization(): every edge is active
  if (s != ORBX_OK) return s;
  L.cap.cur_phase = 0;
  // optimize(n <= 0) runs no iteration, as a raised flag does at the loop head
  static const int kRaised = 1;
  StopFlag none;
  none.i = &kRaised;
  s = L.optimize_dev(std::max(n_iterations, 1), n_iterations > 0 ? stop : none, dstop, st, &res->iterations[0],
                     &res->chi2[0]);
  if (s != ORBX_OK) return s;
  res->trials = L.trials;
  // :228-282 every vertex is written back; there is no erase list (the caller's flags are cleared)
  BA_CHECK(ba_writeback(L, pb, res, true, st, false));
  L.unmap_stop();
  BA_CHECK(hipStreamSynchronize(st));
  ba_writeback_finish(L, pb, res, true, false);
  if (ne > 0 && res->edge_outlier) std::memset(res->edge_outlier, 0, ne);
  return ORBX_OK;
}

}  // namespace orbx

// orbx_plan.h -- the per-geometry plan of the extraction kernels, as the host builds it (plan.hip).
//
// Pure host arithmetic: no HIP runtime call, nothing allocated on a device.  The plan decides every
// LDS size, table index and launch group the kernels of extract.hip use unguarded; an extractor
// handle (orbx_extractor.h) uploads it, tests/cpp/test_plan.cpp walks it under the sanitizers.
#pragma once
#include <vector>

#include "orbx_internal.h"

namespace orbx {

// ORBextractor's constructor tables (src/ORBextractor.cc:416-490)
struct Tables {
  std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
  std::vector<int> nfeat;
  int umax[16];
};

struct Plan {
  Geometry G{};
  std::vector<CellInfo> cells;
  std::vector<int> tile_level;
  std::vector<ResizeX> xt;
  std::vector<ResizeY> yt;
  std::vector<int2> rzb;  // k_resize footprint bounds: per level its tile columns, then its tile rows
  int rzb_x[kMaxLevelsPlan] = {}, rzb_y[kMaxLevelsPlan] = {};  // where a level's two runs start in rzb
  // k_resize_strip's bounds follow k_resize's in rzb (from rzb_n on): a strip level's two runs
  int rzb_n = 0, rsb_x[kMaxLevelsPlan] = {}, rsb_y[kMaxLevelsPlan] = {};
  bool strip[kMaxLevelsPlan] = {};  // the level takes the fast path (strip_resize_ok)
};

bool params_ok(const orbx_extractor_params* p);
Tables make_tables(const orbx_extractor_params& p);
void gaussian_int_kernel(int k[7]);
// ORBX_ERR_SIZE for a geometry no kernel instance serves
orbx_status build_plan(const orbx_extractor_params& p, const Tables& t, int W, int H, Plan& P);
bool strip_resize_ok(const Plan& P, int l);
// k_resize's launch descriptors of a built plan over the given table bases (the device copies in
// use; the host vectors themselves for orbx_debug_launch_plan).  rm is left for the launch.
void build_launch_plan(const Plan& P, const ResizeX* xt, const ResizeY* yt, const int2* rzb, LaunchPlan& LP);

}  // namespace orbx

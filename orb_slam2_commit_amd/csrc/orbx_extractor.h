// orbx_extractor.h -- the extractor handle and the host-path helpers the units that work on it share
// (capi.hip defines the functions; debug.hip is the other user).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <utility>

#include "orbx_mem.h"
#include "orbx_plan.h"
#include "orbx_prof.h"
#include "orbx_scratch.h"
#include "orbx_stereo.h"

namespace orbx {

// A plan as a handle holds it: the host part (orbx_plan.h) and its device copies
struct DevPlan : Plan {
  LaunchPlan LP{};  // k_resize's by-value descriptors, pointing into the device tables below
  DevBuf<Geometry> dG;
  DevBuf<CellInfo> dcells;
  DevBuf<int> dtiles;
  DevBuf<ResizeX> dxt;
  DevBuf<ResizeY> dyt;
  DevBuf<int2> drzb;
};

// Offsets of a device block's fields: they start behind the 256-byte counts header, each at the next
// scratch_align-ed offset in take() order; end() is the block's size.
struct BlockCursor {
  size_t at = 256;
  template <class T>
  size_t take(size_t count) {
    const size_t o = at;
    at += scratch_align(count * sizeof(T));
    return o;
  }
  size_t end() const { return at; }
};

// `rows` rows of row_bytes each, `stride` apart at src, packed back to back at dst
inline void pack_rows(uint8_t* dst, const void* src, size_t stride, size_t row_bytes, int rows) {
  for (int y = 0; y < rows; y++) std::memcpy(dst + (size_t)y * row_bytes, (const uint8_t*)src + (size_t)y * stride, row_bytes);
}

// an optional output array of a host API
inline void copy_out(void* dst, const void* src, size_t bytes) {
  if (dst) std::memcpy(dst, src, bytes);
}

// One side of the stereo matcher's input (StereoArgs' per-side fields): frame f's keypoints at
// kps + f * k_stride, its count at counts[f * n_stride], its pyramid image step * f + off of the batch.
struct StereoSide {
  const orbx_keypoint* kps;
  const uint8_t* desc;
  const int32_t* counts;
  long long k_stride, n_stride;
  int step, off;
};
struct StereoSides {
  StereoSide L, R;
  // one frame, each side the output of a handle's own extraction: strides 0
  static StereoSides handles(const orbx_keypoint* kL, const uint8_t* dL, const int32_t* nL, const orbx_keypoint* kR,
                             const uint8_t* dR, const int32_t* nR) {
    return {{kL, dL, nL, 0, 0, 0, 0}, {kR, dR, nR, 0, 0, 0, 0}};
  }
  // an interleaved batch of 2n images (left, right, left, ...) extracted at keypoint capacity kc
  static StereoSides interleaved(const orbx_keypoint* kps, const uint8_t* desc, const int32_t* counts, long long kc) {
    return {{kps, desc, counts, 2 * kc, 2, 2, 0}, {kps + kc, desc + kc * 32, counts + 1, 2 * kc, 2, 2, 1}};
  }
};

}  // namespace orbx

struct orbx_extractor {
  orbx_extractor_params params{};
  int device = 0;
  hipStream_t stream = nullptr;
  orbx::Tables tables;
  std::map<std::pair<int, int>, std::unique_ptr<orbx::DevPlan>> plans;
  // batch buffers
  orbx::DevBuf<uint8_t> pyr, blur;
  orbx::DevBuf<uint32_t> cand, kpos, oct;
  orbx::DevBuf<int> cell_count, knode, oct_count;
  // host-API staging: the input image, and ONE output block [count | keypoints | descriptors]
  // (orbx_extract reads it back with one copy; orbx_stereo_match reads it in place)
  orbx::DevBuf<uint8_t> in, out;
  size_t out_kps = 0, out_desc = 0, out_bytes = 0;
  orbx::PinnedBuf hstage;  // the input image on the way in, the output block on the way out
  // stereo scratch
  orbx::DevBuf<uint64_t> rkeys;
  orbx::DevBuf<int2> rxi;
  orbx::DevBuf<uint4> rdesc;
  orbx::DevBuf<uint32_t> rtab;
  orbx::DevBuf<uint4> lrange;
  orbx::DevBuf<int> oct_start, sad;
  orbx::DevBuf<float> sres;  // orbx_stereo_match: uRight | depth, adjacent (one copy back)
  orbx::DevBuf<int32_t> nmatch;
  // RGB-D: orbx_frame_rgbd's upload [image | depth image]; the out-of-image counters of a device batch.
  // (The grey images of a colour input go into `in`: level 0 of that call's pyramid.)
  orbx::DevBuf<uint8_t> rgbd_in;
  orbx::DevBuf<int32_t> rgbd_oob;
  orbx::StageTimer timer;
  // last batch (mvImagePyramid)
  orbx::DevPlan* last_plan = nullptr;
  const uint8_t* last_in = nullptr;
  size_t last_pitch = 0;
  int last_n = 0;
  // fingerprint of the keypoints the last host-API orbx_extract returned: orbx_stereo_match only
  // reads this handle's pyramid for exactly those keypoints (a batch extraction clears it)
  bool last_host = false;
  int last_fp_n = 0;
  uint64_t last_fp = 0;
  // mvImagePyramid readback (orbx_extractor_set_pyramid_readback): level 0 (the packed input) then
  // levels 1.. exactly as packed on the device, in pinned memory; valid for the last orbx_extract
  bool pyr_readback = false;
  bool hpyr_valid = false;
  orbx::PinnedBuf hpyr;
  size_t hpyr_l0 = 0;
};

namespace orbx {

inline orbx_status hip_status(hipError_t e) { return e == hipSuccess ? ORBX_OK : ORBX_ERR_HIP; }
inline hipStream_t pick_stream(orbx_extractor* h, void* s) {
  return s == ORBX_STREAM_NULL ? (hipStream_t)0 : s ? (hipStream_t)s : h->stream;
}
orbx_status get_plan(orbx_extractor* h, int W, int H, DevPlan** out);
orbx_status ensure_batch(orbx_extractor* h, const Plan& P, int n);
BatchPtrs batch_ptrs(orbx_extractor* h, const uint8_t* in, size_t pitch);
orbx_status run_extract(orbx_extractor* h, DevPlan* P, int n, const uint8_t* d_in, size_t pitch, orbx_keypoint* d_kps,
                        uint8_t* d_desc, int32_t* d_counts, int kp_cap, hipStream_t st);
// The matcher on n_frames frames of S through hl's scratch, the pyramids those of hl's and hr's last
// batches; outputs per frame at stride out_stride.
orbx_status run_stereo(orbx_extractor* hl, orbx_extractor* hr, int n_frames, const StereoSides& S, int maxL, float bf,
                       float baseline, float* uR, float* depth, long long out_stride, int32_t* nmatches,
                       hipStream_t st);

}  // namespace orbx

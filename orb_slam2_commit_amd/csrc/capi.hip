// capi.hip -- the extractor handle's host side: its part of the C ABI declared in include/orbx.h.
//
// An orbx_extractor (orbx_extractor.h) owns: one HIP stream, the parameter tables of the
// reference constructor (src/ORBextractor.cc:416-490), a plan per image
// geometry (built on the host by plan.hip, uploaded here), and device buffers grown to the largest
// batch seen.  This unit holds the handle's shared paths (get_plan, run_extract, run_stereo) and its
// entry points: create / destroy and the table getters, extraction, the pyramid readback, the stereo
// and RGB-D front ends, the stage profile; and the library's version, sizeof, device count and
// descriptor distance.  No kernels, and nothing here computes results on the CPU: every output comes
// from the HIP kernels in extract.hip / stereo.hip / rgbd.hip.  (orbx_debug_* is debug.hip.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <string>

#include "orbx_extractor.h"
#include "orbx_rgbd.h"
#include "orbx_undistort.h"

namespace orbx {

orbx_status get_plan(orbx_extractor* h, int W, int H, DevPlan** out) {
  auto key = std::make_pair(W, H);
  auto it = h->plans.find(key);
  if (it != h->plans.end()) {
    *out = it->second.get();
    return ORBX_OK;
  }
  std::unique_ptr<DevPlan> P(new (std::nothrow) DevPlan());
  if (!P) return ORBX_ERR_HIP;
  orbx_status s = build_plan(h->params, h->tables, W, H, *P);
  if (s != ORBX_OK) return s;
  hipError_t e = P->dG.upload(&P->G, 1);
  if (e == hipSuccess) e = P->dcells.upload(P->cells.data(), P->cells.size());
  if (e == hipSuccess) e = P->dtiles.upload(P->tile_level.data(), P->tile_level.size());
  if (e == hipSuccess) e = P->drzb.upload(P->rzb.data(), P->rzb.size());
  if (e == hipSuccess) e = P->dxt.upload(P->xt.data(), P->xt.size());
  if (e == hipSuccess) e = P->dyt.upload(P->yt.data(), P->yt.size());
  if (e != hipSuccess) return ORBX_ERR_HIP;
  build_launch_plan(*P, P->dxt.p, P->dyt.p, P->drzb.p, P->LP);
  size_t mx = octree_group_smem(P->G.og_all);
  for (int g = 0; g < P->G.n_og; g++) mx = std::max(mx, octree_group_smem(P->G.og[g]));
  if (octree_set_smem_limit(mx) != hipSuccess) return ORBX_ERR_HIP;
  *out = P.get();
  h->plans[key] = std::move(P);
  return ORBX_OK;
}

orbx_status ensure_batch(orbx_extractor* h, const Plan& P, int n) {
  const Geometry& G = P.G;
  hipError_t e = hipSuccess;
  auto chk = [&](hipError_t x) { if (x != hipSuccess) e = x; };
  chk(h->pyr.ensure((size_t)G.pyr_bytes * n + 256));
  chk(h->blur.ensure((size_t)G.blur_bytes * n + 256));
  chk(h->cand.ensure((size_t)G.cand_total * n));
  chk(h->kpos.ensure((size_t)G.cand_total * n));
  chk(h->knode.ensure((size_t)G.cand_total * n));
  chk(h->cell_count.ensure((size_t)std::max(G.ncells, 1) * n));
  chk(h->oct.ensure((size_t)G.oct_total * n));
  chk(h->oct_count.ensure((size_t)G.nlevels * n));
  return hip_status(e);
}

BatchPtrs batch_ptrs(orbx_extractor* h, const uint8_t* in, size_t pitch) {
  BatchPtrs B;
  B.in = in;
  B.in_pitch = pitch;
  B.pyr = h->pyr.p;
  B.blur = h->blur.p;
  B.cand = h->cand.p;
  B.cell_count = h->cell_count.p;
  B.kpos = h->kpos.p;
  B.knode = h->knode.p;
  B.oct = h->oct.p;
  B.oct_count = h->oct_count.p;
  return B;
}

orbx_status run_extract(orbx_extractor* h, DevPlan* P, int n, const uint8_t* d_in, size_t pitch, orbx_keypoint* d_kps,
                        uint8_t* d_desc, int32_t* d_counts, int kp_cap, hipStream_t st) {
  if (kp_cap < P->G.max_kps) return ORBX_ERR_CAPACITY;
  orbx_status s = ensure_batch(h, *P, n);
  if (s != ORBX_OK) return s;
  BatchPtrs B = batch_ptrs(h, d_in, pitch);
  hipError_t e = launch_extract_stages(P->G, P->dG.p, P->dcells.p, P->dtiles.p, P->LP, B, n, d_kps, d_desc, d_counts, kp_cap, st,
                                       &h->timer);
  if (e != hipSuccess) return ORBX_ERR_HIP;
  h->last_plan = P;
  h->last_in = d_in;
  h->last_pitch = pitch;
  h->last_n = n;
  h->last_host = false;  // orbx_extract sets it again after its readback
  h->hpyr_valid = false;
  return ORBX_OK;
}

orbx_status run_stereo(orbx_extractor* hl, orbx_extractor* hr, int n_frames, const StereoSides& S, int maxL, float bf,
                       float baseline, float* uR, float* depth, long long out_stride, int32_t* nmatches,
                       hipStream_t st) {
  orbx_extractor* h = hl;
  const DevPlan* P = hl->last_plan;
  hipError_t e = hipSuccess;
  auto chk = [&](hipError_t x) { if (x != hipSuccess) e = x; };
  chk(h->rkeys.ensure((size_t)n_frames * kMaxStereoKps));
  chk(h->oct_start.ensure((size_t)n_frames * (kMaxLevelsPlan + 1)));
  chk(h->rxi.ensure((size_t)n_frames * kMaxStereoKps));
  chk(h->rdesc.ensure((size_t)n_frames * kMaxStereoKps * 2));
  chk(h->rtab.ensure((size_t)n_frames * P->G.nlevels * std::max(P->G.height, 1)));
  chk(h->lrange.ensure((size_t)n_frames * std::max(maxL, 1)));
  chk(h->sad.ensure((size_t)n_frames * out_stride));
  if (e != hipSuccess) return ORBX_ERR_HIP;
  StereoArgs A;
  std::memset(&A, 0, sizeof(A));
  A.kpL = S.L.kps;
  A.dL = S.L.desc;
  A.nL = S.L.counts;
  A.kL_stride = S.L.k_stride;
  A.n_stride_L = S.L.n_stride;
  A.l_step = S.L.step;
  A.l_off = S.L.off;
  A.kpR = S.R.kps;
  A.dR = S.R.desc;
  A.nR = S.R.counts;
  A.kR_stride = S.R.k_stride;
  A.n_stride_R = S.R.n_stride;
  A.r_step = S.R.step;
  A.r_off = S.R.off;
  A.BL = batch_ptrs(hl, hl->last_in, hl->last_pitch);
  A.BR = batch_ptrs(hr, hr->last_in, hr->last_pitch);
  A.nlevels = P->G.nlevels;
  A.maxL = maxL;
  for (int l = 0; l < P->G.nlevels; l++) A.inv_scale[l] = hl->tables.inv_scale[l];
  A.bf = bf;
  A.minZ = baseline;
  A.minD = 0.f;
  A.maxD = bf / baseline;  // mbf/minZ, src/Frame.cc:595-597
  A.uR = uR;
  A.depth = depth;
  A.sad = h->sad.p;
  A.out_stride = out_stride;
  A.rkeys = h->rkeys.p;
  A.oct_start = h->oct_start.p;
  A.rxi = h->rxi.p;
  A.rdesc = h->rdesc.p;
  A.rtab = h->rtab.p;
  A.lrange = h->lrange.p;
  A.rows = std::max(P->G.height, 1);
  A.nmatches = nmatches;
  return hip_status(launch_stereo(A, P->dG.p, n_frames, maxL, st, &h->timer));
}

}  // namespace orbx

using namespace orbx;

namespace {

// Bytes past the last pixel of the handle's input buffer.  k_stereo_match stages its SAD rows with
// dword loads from the 4-aligned address at or below a row's first byte, so it reads up to 3 bytes past
// a row's last needed one; at the bottom-right patch of level 0 (which is the input buffer) that is
// up to 3 bytes past the image.  The pyramid buffer carries 256 bytes of slack for the same reason.
constexpr size_t kInSlack = 4;

// 64-bit fingerprint of n keypoint records and their descriptors (multiply-xorshift over 32-bit
// words, a few microseconds for 2,000 keypoints): orbx_stereo_match uses the device copies of the
// extraction only when the caller hands back exactly what that extraction returned
uint64_t fingerprint_words(const void* p, size_t nw, uint64_t h) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
  for (size_t i = 0; i < nw; i++) {
    h = (h ^ w[i]) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
  }
  return h;
}
uint64_t keypoint_fingerprint(const orbx_keypoint* k, const uint8_t* desc, int n) {
  uint64_t h = 1469598103934665603ull ^ (uint64_t)n;
  h = fingerprint_words(k, (size_t)n * (sizeof(orbx_keypoint) / 4), h);
  if (desc) h = fingerprint_words(desc, (size_t)n * 8, h ^ 0xD6E8FEB86659FD93ull);
  return h;
}


}  // namespace

extern "C" {

const char* orbx_version(void) { return "orbx 0.1.0 (gfx950)"; }

long long orbx_sizeof(const char* type) {
  if (!type) return -1;
  const std::string t(type);
#define ORBX_SIZEOF(T) \
  if (t == #T) return (long long)sizeof(T);
  ORBX_SIZEOF(orbx_keypoint) ORBX_SIZEOF(orbx_extractor_params) ORBX_SIZEOF(orbx_bow_side)
  ORBX_SIZEOF(orbx_bow_problem) ORBX_SIZEOF(orbx_ba_problem) ORBX_SIZEOF(orbx_ba_result)
  ORBX_SIZEOF(orbx_pnp_problem) ORBX_SIZEOF(orbx_pnp_params) ORBX_SIZEOF(orbx_pnp_result)
  ORBX_SIZEOF(orbx_rand_state) ORBX_SIZEOF(orbx_proj_frame) ORBX_SIZEOF(orbx_proj_problem)
  ORBX_SIZEOF(orbx_tri_kf) ORBX_SIZEOF(orbx_tri_problem) ORBX_SIZEOF(orbx_pose_problem)
  ORBX_SIZEOF(orbx_track_gather) ORBX_SIZEOF(orbx_frame_points) ORBX_SIZEOF(orbx_track_step)
  ORBX_SIZEOF(orbx_camera) ORBX_SIZEOF(orbx_sim3_problem) ORBX_SIZEOF(orbx_init_problem)
  ORBX_SIZEOF(orbx_sim3_solver_problem) ORBX_SIZEOF(orbx_sim3_params) ORBX_SIZEOF(orbx_sim3_result)
  ORBX_SIZEOF(orbx_optimize_sim3_problem) ORBX_SIZEOF(orbx_essential_graph_problem)
  ORBX_SIZEOF(orbx_essential_graph_result) ORBX_SIZEOF(orbx_new_points_kf)
  ORBX_SIZEOF(orbx_new_points_problem) ORBX_SIZEOF(orbx_new_points_result)
#undef ORBX_SIZEOF
  return -1;
}

int orbx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

orbx_status orbx_extractor_create(const orbx_extractor_params* params, int device, orbx_extractor** out) {
  if (!out || !params_ok(params)) return ORBX_ERR_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ORBX_ERR_NODEV;
  if (device < 0 || device >= n) return ORBX_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return ORBX_ERR_HIP;
  orbx_extractor* h = new (std::nothrow) orbx_extractor();
  if (!h) return ORBX_ERR_HIP;
  h->params = *params;
  h->device = device;
  h->tables = make_tables(*params);
  int gauss[7];
  gaussian_int_kernel(gauss);
  if (upload_constants(h->tables.umax, gauss) != hipSuccess ||
      hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return ORBX_ERR_HIP;
  }
  *out = h;
  return ORBX_OK;
}

void orbx_extractor_destroy(orbx_extractor* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamDestroy(h->stream);
  }
  delete h;
}

int orbx_extractor_get_levels(const orbx_extractor* h) { return h ? h->params.nlevels : ORBX_ERR_ARG; }

orbx_status orbx_extractor_scale_tables(const orbx_extractor* h, float* scale, float* inv_scale, float* sigma2,
                                        float* inv_sigma2) {
  if (!h) return ORBX_ERR_ARG;
  const int n = h->params.nlevels;
  for (int i = 0; i < n; i++) {
    if (scale) scale[i] = h->tables.scale[i];
    if (inv_scale) inv_scale[i] = h->tables.inv_scale[i];
    if (sigma2) sigma2[i] = h->tables.sigma2[i];
    if (inv_sigma2) inv_sigma2[i] = h->tables.inv_sigma2[i];
  }
  return ORBX_OK;
}

orbx_status orbx_extractor_tables(const orbx_extractor* h, int* features_per_level, int* umax, int* pattern) {
  if (!h) return ORBX_ERR_ARG;
  static const int8_t kPattern[512 * 2] = {
#include "brief_pattern_31.inc"
  };
  for (int i = 0; i < h->params.nlevels; i++)
    if (features_per_level) features_per_level[i] = h->tables.nfeat[i];
  for (int v = 0; v < 16; v++)
    if (umax) umax[v] = h->tables.umax[v];
  for (int i = 0; i < 1024; i++)
    if (pattern) pattern[i] = kPattern[i];
  return ORBX_OK;
}

orbx_status orbx_extractor_set_pyramid_readback(orbx_extractor* h, int on) {
  if (!h) return ORBX_ERR_ARG;
  h->pyr_readback = on != 0;
  if (!h->pyr_readback) h->hpyr_valid = false;
  return ORBX_OK;
}

int orbx_extractor_max_keypoints(orbx_extractor* h, int width, int height) {
  if (!h) return ORBX_ERR_ARG;
  DevPlan* P = nullptr;
  orbx_status s = get_plan(h, width, height, &P);
  return s == ORBX_OK ? P->G.max_kps : s;
}

orbx_status orbx_extract(orbx_extractor* h, const uint8_t* img, int width, int height, size_t stride,
                         orbx_keypoint* kps, int cap, uint8_t* desc, int* n) {
  if (!h || !n) return ORBX_ERR_ARG;
  *n = 0;
  if (!img || width <= 0 || height <= 0) return ORBX_OK;  // src/ORBextractor.cc:1141
  if (stride < (size_t)width) return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  DevPlan* P = nullptr;
  orbx_status s = get_plan(h, width, height, &P);
  if (s != ORBX_OK) return s;
  const int kcap = P->G.max_kps;
  hipError_t e = hipSuccess;
  auto chk = [&](hipError_t x) { if (x != hipSuccess) e = x; };
  const size_t npx = (size_t)width * height;
  BlockCursor blk;
  h->out_kps = blk.take<orbx_keypoint>(kcap);
  h->out_desc = blk.take<uint8_t>((size_t)kcap * 32);
  h->out_bytes = blk.end();
  chk(h->in.ensure(npx + kInSlack));
  chk(h->out.ensure(h->out_bytes));
  chk(h->hstage.ensure(std::max(npx, h->out_bytes)));
  if (e != hipSuccess) return ORBX_ERR_HIP;
  hipStream_t st = h->stream;
  uint8_t* hs = h->hstage.p;
  // the image through pinned staging (a pageable copy is staged by the runtime, synchronously)
  pack_rows(hs, img, stride, width, height);
  if (hipMemcpyAsync(h->in.p, hs, npx, hipMemcpyHostToDevice, st) != hipSuccess) return ORBX_ERR_HIP;
  int32_t* d_count = (int32_t*)h->out.p;
  orbx_keypoint* d_kps = (orbx_keypoint*)(h->out.p + h->out_kps);
  uint8_t* d_desc = h->out.p + h->out_desc;
  s = run_extract(h, P, 1, h->in.p, npx, d_kps, d_desc, d_count, kcap, st);
  if (s != ORBX_OK) return s;
  const bool pyr = h->pyr_readback;
  if (pyr) {
    // mvImagePyramid (src/ORBextractor.cc:1215-1250 rebuilds it on every call): levels 1.. leave in
    // one more D2H behind the output block; level 0 is the staged input, copied on the host while
    // the kernels run
    h->hpyr_l0 = scratch_align(npx);
    if (h->hpyr.ensure(h->hpyr_l0 + (size_t)P->G.pyr_bytes) != hipSuccess) return ORBX_ERR_HIP;
  }
  // count, keypoints and descriptors in ONE copy, then the stream's only synchronisation
  chk(hipMemcpyAsync(hs, h->out.p, h->out_bytes, hipMemcpyDeviceToHost, st));
  if (pyr && P->G.nlevels > 1)
    chk(hipMemcpyAsync(h->hpyr.p + h->hpyr_l0, h->pyr.p, (size_t)P->G.pyr_bytes, hipMemcpyDeviceToHost, st));
  if (pyr) pack_rows(h->hpyr.p, img, stride, width, height);  // from the caller's image (hstage is the output's destination by now)
  chk(hipStreamSynchronize(st));
  if (e != hipSuccess) return ORBX_ERR_HIP;
  const int32_t cnt = *(const int32_t*)hs;
  *n = cnt;
  if (cnt > cap) return ORBX_ERR_CAPACITY;
  const orbx_keypoint* hk = (const orbx_keypoint*)(hs + h->out_kps);
  copy_out(kps, hk, sizeof(orbx_keypoint) * cnt);
  copy_out(desc, hs + h->out_desc, (size_t)32 * cnt);
  h->last_host = true;
  h->hpyr_valid = pyr;
  h->last_fp_n = cnt;
  h->last_fp = keypoint_fingerprint(hk, hs + h->out_desc, cnt);
  return ORBX_OK;
}

orbx_status orbx_pyramid_level(orbx_extractor* h, int image, int level, uint8_t* dst, size_t dst_stride,
                               int* width, int* height) {
  if (!h) return ORBX_ERR_ARG;
  if (!h->last_plan) return ORBX_ERR_STATE;
  const Geometry& G = h->last_plan->G;
  if (level < 0 || level >= G.nlevels || image < 0 || image >= h->last_n) return ORBX_ERR_ARG;
  const int w = G.lv[level].w, hh = G.lv[level].h;
  if (width) *width = w;
  if (height) *height = hh;
  if (!dst) return ORBX_OK;
  if (dst_stride < (size_t)w) return ORBX_ERR_ARG;
  if (h->hpyr_valid && image == 0) {
    // staged by the last orbx_extract: a host copy, no device call
    const uint8_t* src = level == 0 ? h->hpyr.p : h->hpyr.p + h->hpyr_l0 + G.lv[level].off;
    for (int y = 0; y < hh; y++) std::memcpy(dst + (size_t)y * dst_stride, src + (size_t)y * w, w);
    return ORBX_OK;
  }
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  BatchPtrs B = batch_ptrs(h, h->last_in, h->last_pitch);
  const uint8_t* src = level_ptr(G, B, image, level);
  hipError_t e = hipMemcpy2DAsync(dst, dst_stride, src, w, w, hh, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  return hip_status(e);
}

orbx_status orbx_extract_batch_device(orbx_extractor* h, int n_images, const uint8_t* d_images, int width,
                                      int height, size_t image_pitch, orbx_keypoint* d_kps, uint8_t* d_desc,
                                      int32_t* d_counts, int kp_capacity, void* stream) {
  if (!h || n_images < 0 || !d_kps || !d_desc || !d_counts) return ORBX_ERR_ARG;
  if (n_images == 0) return ORBX_OK;
  if (!d_images || width <= 0 || height <= 0 || image_pitch < (size_t)width * height) return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  DevPlan* P = nullptr;
  orbx_status s = get_plan(h, width, height, &P);
  if (s != ORBX_OK) return s;
  return run_extract(h, P, n_images, d_images, image_pitch, d_kps, d_desc, d_counts, kp_capacity,
                     pick_stream(h, stream));
}

orbx_status orbx_stereo_match(orbx_extractor* left, orbx_extractor* right, const orbx_keypoint* kpsL,
                              const uint8_t* descL, int nL, const orbx_keypoint* kpsR, const uint8_t* descR,
                              int nR, float bf, float baseline, float* uRight, float* depth) {
  if (!left || !right || !uRight || !depth || nL < 0 || nR < 0) return ORBX_ERR_ARG;
  if ((nL > 0 && (!kpsL || !descL)) || (nR > 0 && (!kpsR || !descR))) return ORBX_ERR_ARG;
  if (!left->last_plan || !right->last_plan) return ORBX_ERR_STATE;
  // the pyramids must belong to the supplied keypoints: each handle's last call was orbx_extract and
  // returned exactly these keypoints (src/Frame.cc:556,681 read mpORBextractorLeft/Right->mvImagePyramid
  // of the extraction that produced mvKeys/mvKeysRight)
  if (!left->last_host || !right->last_host || nL != left->last_fp_n || nR != right->last_fp_n ||
      (nL > 0 && keypoint_fingerprint(kpsL, descL, nL) != left->last_fp) ||
      (nR > 0 && keypoint_fingerprint(kpsR, descR, nR) != right->last_fp))
    return ORBX_ERR_STATE;
  if (left->last_plan->G.width != right->last_plan->G.width ||
      left->last_plan->G.height != right->last_plan->G.height || left->device != right->device)
    return ORBX_ERR_ARG;
  if (nR > kMaxStereoKps) return ORBX_ERR_CAPACITY;
  if (nL == 0) return ORBX_OK;
  orbx_extractor* h = left;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  hipError_t e = hipSuccess;
  auto chk = [&](hipError_t x) { if (x != hipSuccess) e = x; };
  chk(h->sres.ensure(2 * (size_t)nL));
  chk(h->nmatch.ensure(1));
  chk(h->hstage.ensure((size_t)8 * nL));
  if (e != hipSuccess) return ORBX_ERR_HIP;
  hipStream_t st = h->stream;
  // The keypoints and descriptors are the ones each handle's last orbx_extract left on the device
  // (the fingerprints above prove it): no upload.  orbx_extract synchronised both streams before
  // returning them, so the right handle's block and pyramid are complete.
  const uint8_t *bL = left->out.p, *bR = right->out.p;
  const StereoSides S = StereoSides::handles((const orbx_keypoint*)(bL + left->out_kps), bL + left->out_desc,
                                             (const int32_t*)bL, (const orbx_keypoint*)(bR + right->out_kps),
                                             bR + right->out_desc, (const int32_t*)bR);
  orbx_status s = run_stereo(left, right, 1, S, nL, bf, baseline, h->sres.p, h->sres.p + nL, nL, h->nmatch.p, st);
  if (s != ORBX_OK) return s;
  chk(hipMemcpyAsync(h->hstage.p, h->sres.p, sizeof(float) * 2 * nL, hipMemcpyDeviceToHost, st));
  chk(hipStreamSynchronize(st));
  if (e != hipSuccess) return ORBX_ERR_HIP;
  copy_out(uRight, h->hstage.p, sizeof(float) * nL);
  copy_out(depth, h->hstage.p + sizeof(float) * nL, sizeof(float) * nL);
  return ORBX_OK;
}

orbx_status orbx_frame_stereo(orbx_extractor* h, const uint8_t* imL, size_t strideL, const uint8_t* imR,
                              size_t strideR, int width, int height, float bf, float baseline, orbx_keypoint* kpsL,
                              uint8_t* descL, int capL, int* nL, orbx_keypoint* kpsR, uint8_t* descR, int capR,
                              int* nR, float* uRight, float* depth) {
  if (!h || !nL || !nR) return ORBX_ERR_ARG;
  *nL = *nR = 0;
  if (!imL || !imR || width <= 0 || height <= 0) return ORBX_ERR_ARG;
  if (strideL < (size_t)width || strideR < (size_t)width) return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  DevPlan* P = nullptr;
  orbx_status s = get_plan(h, width, height, &P);
  if (s != ORBX_OK) return s;
  const int kc = P->G.max_kps;
  if (kc > kMaxStereoKps) return ORBX_ERR_CAPACITY;
  // device output block: counts (L, R) and the match count | keypoints (L | R, kc each) |
  // descriptors (L | R) | uRight | depth -- one copy back; the images go in as a batch of two
  const size_t npx = (size_t)width * height;
  BlockCursor blk;
  const size_t o_kps = blk.take<orbx_keypoint>((size_t)2 * kc), o_desc = blk.take<uint8_t>((size_t)2 * kc * 32),
               o_ur = blk.take<float>(kc), o_dep = blk.take<float>(kc), o_end = blk.end();
  hipError_t e = hipSuccess;
  auto chk = [&](hipError_t x) { if (x != hipSuccess) e = x; };
  chk(h->in.ensure(2 * npx + kInSlack));
  chk(h->out.ensure(o_end));
  chk(h->hstage.ensure(std::max(2 * npx, o_end)));
  if (e != hipSuccess) return ORBX_ERR_HIP;
  hipStream_t st = h->stream;
  // the left image's copy runs while the right one is staged
  uint8_t* hs = h->hstage.p;
  pack_rows(hs, imL, strideL, width, height);
  chk(hipMemcpyAsync(h->in.p, hs, npx, hipMemcpyHostToDevice, st));
  pack_rows(hs + npx, imR, strideR, width, height);
  chk(hipMemcpyAsync(h->in.p + npx, hs + npx, npx, hipMemcpyHostToDevice, st));
  if (e != hipSuccess) return ORBX_ERR_HIP;
  int32_t* d_counts = (int32_t*)h->out.p;
  orbx_keypoint* d_kps = (orbx_keypoint*)(h->out.p + o_kps);
  uint8_t* d_desc = h->out.p + o_desc;
  s = run_extract(h, P, 2, h->in.p, npx, d_kps, d_desc, d_counts, kc, st);
  if (s != ORBX_OK) return s;
  // images 0 (left) and 1 (right) of the batch
  s = run_stereo(h, h, 1, StereoSides::interleaved(d_kps, d_desc, d_counts, kc), kc, bf, baseline,
                 (float*)(h->out.p + o_ur), (float*)(h->out.p + o_dep), kc, d_counts + 2, st);
  if (s != ORBX_OK) return s;
  chk(hipMemcpyAsync(hs, h->out.p, o_end, hipMemcpyDeviceToHost, st));
  chk(hipStreamSynchronize(st));
  if (e != hipSuccess) return ORBX_ERR_HIP;
  // this handle's block no longer holds a single orbx_extract result (orbx_stereo_match refuses it);
  // orbx_pyramid_level serves images 0 / 1 of this batch from the device
  h->last_host = false;
  h->hpyr_valid = false;
  const int cl = ((const int32_t*)hs)[0], cr = ((const int32_t*)hs)[1];
  *nL = cl;
  *nR = cr;
  if (cl > capL || cr > capR) return ORBX_ERR_CAPACITY;
  const orbx_keypoint* hk = (const orbx_keypoint*)(hs + o_kps);
  copy_out(kpsL, hk, sizeof(orbx_keypoint) * cl);
  copy_out(descL, hs + o_desc, (size_t)32 * cl);
  copy_out(uRight, hs + o_ur, sizeof(float) * cl);
  copy_out(depth, hs + o_dep, sizeof(float) * cl);
  copy_out(kpsR, hk + kc, sizeof(orbx_keypoint) * cr);
  copy_out(descR, hs + o_desc + (size_t)kc * 32, (size_t)32 * cr);
  return ORBX_OK;
}

orbx_status orbx_stereo_frames_device(orbx_extractor* h, int n_frames, const uint8_t* d_images, int width,
                                      int height, size_t image_pitch, orbx_keypoint* d_kps, uint8_t* d_desc,
                                      int32_t* d_counts, int kp_capacity, float bf, float baseline,
                                      float* d_uright, float* d_depth, int32_t* d_nmatches, void* stream) {
  if (!h || n_frames < 0 || !d_uright || !d_depth || !d_nmatches) return ORBX_ERR_ARG;
  if (n_frames == 0) return ORBX_OK;
  orbx_status s = orbx_extract_batch_device(h, 2 * n_frames, d_images, width, height, image_pitch, d_kps, d_desc,
                                            d_counts, kp_capacity, stream);
  if (s != ORBX_OK) return s;
  if (h->last_plan->G.max_kps > kMaxStereoKps) return ORBX_ERR_CAPACITY;
  return run_stereo(h, h, n_frames, StereoSides::interleaved(d_kps, d_desc, d_counts, kp_capacity),
                    h->last_plan->G.max_kps, bf, baseline, d_uright, d_depth, kp_capacity, d_nmatches,
                    pick_stream(h, stream));
}

// ------------------------------------------------------------------ RGB-D front end (kernels: rgbd.hip)
namespace {

// src/Tracking.cc:230: `fabs(mDepthMapFactor-1.0f)>1e-5`, a float subtraction then a double comparison
bool depth_factor_applies(float factor) { return (double)std::fabs(factor - 1.0f) > 1e-5; }

size_t depth_elem(int type) { return type == ORBX_DEPTH_U16 ? 2 : type == ORBX_DEPTH_F32 ? 4 : 0; }

// bytes from the first byte of image 0 to the last byte of the last row of image n - 1
size_t span_bytes(size_t row_bytes, size_t pitch, int h, size_t image_pitch, int n) {
  return (size_t)(n - 1) * image_pitch + (size_t)(h - 1) * pitch + row_bytes;
}

orbx_status cvt_gray_check(const void* src, size_t sp, size_t sip, int n, int w, int h, int ch, const void* dst,
                           size_t dp, size_t dip) {
  if (ch != 3 && ch != 4) return ORBX_ERR_ARG;  // 1: the reference does not call cvtColor
  if (n < 0 || w < 0 || h < 0) return ORBX_ERR_ARG;
  if (n == 0 || w == 0 || h == 0) return ORBX_OK;
  if (!src || !dst || sp < (size_t)ch * w || dp < (size_t)w) return ORBX_ERR_ARG;
  if (n > 1 && (sip < span_bytes((size_t)ch * w, sp, h, 0, 1) || dip < span_bytes((size_t)w, dp, h, 0, 1)))
    return ORBX_ERR_ARG;
  if (n > 65535 || h > 4 * 65535) return ORBX_ERR_SIZE;  // k_cvt_gray's grid
  return ORBX_OK;
}

CvtGrayArgs cvt_gray_args(const uint8_t* src, size_t sp, size_t sip, int n, int w, int h, int rgb, uint8_t* dst,
                          size_t dp, size_t dip) {
  CvtGrayArgs A;
  A.src = src;
  A.dst = dst;
  A.src_pitch = (long long)sp;
  A.src_image_pitch = (long long)sip;
  A.dst_pitch = (long long)dp;
  A.dst_image_pitch = (long long)dip;
  A.w = w;
  A.h = h;
  A.n = n;
  A.c0 = rgb ? kR2Y : kB2Y;
  A.c2 = rgb ? kB2Y : kR2Y;
  return A;
}

// k_rgbd_finish behind an extraction of n_frames images through h (kps at stride kc, counts at stride 1)
struct DepthImages {  // device depth images of w x h elements of `type`, divided by `factor` where it applies
  const uint8_t* p;
  size_t pitch, image_pitch;
  int type, w, h;
  float factor;
};
struct RgbdOutputs {
  orbx_keypoint* kps_un;
  float *ur, *dep;
  int32_t *nmatches, *oob;
};
orbx_status run_rgbd_finish(int n_frames, const orbx_keypoint* d_kps, const int32_t* d_counts, long long kc, int max_k,
                            const orbx_camera& cam, float bf, const DepthImages& D, const RgbdOutputs& O,
                            hipStream_t st) {
  RgbdFinishArgs A;
  std::memset(&A, 0, sizeof(A));
  A.kps = d_kps;
  A.counts = d_counts;
  A.k_stride = kc;
  A.n_stride = 1;
  A.max_k = max_k;
  A.cam = cam;
  A.depth = D.p;
  A.depth_pitch = (long long)D.pitch;
  A.depth_image_pitch = (long long)D.image_pitch;
  A.depth_type = D.type;
  A.scale = depth_factor_applies(D.factor) ? 1 : 0;
  A.factor = D.factor;
  A.bf = bf;
  A.w = D.w;
  A.h = D.h;
  A.kps_un = O.kps_un;
  A.uR = O.ur;
  A.dep = O.dep;
  A.out_stride = kc;
  A.nmatches = O.nmatches;
  A.n_oob = O.oob;
  return hip_status(launch_rgbd_finish(A, n_frames, st));
}

}  // namespace

orbx_status orbx_cvt_gray_device(orbx_extractor* h, const uint8_t* d_src, size_t src_pitch, size_t src_image_pitch,
                                 int n_images, int width, int height, int channels, int rgb, uint8_t* d_dst,
                                 size_t dst_pitch, size_t dst_image_pitch, void* stream) {
  if (!h) return ORBX_ERR_ARG;
  const orbx_status s =
      cvt_gray_check(d_src, src_pitch, src_image_pitch, n_images, width, height, channels, d_dst, dst_pitch, dst_image_pitch);
  if (s != ORBX_OK || n_images == 0 || width == 0 || height == 0) return s;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  return hip_status(launch_cvt_gray(cvt_gray_args(d_src, src_pitch, src_image_pitch, n_images, width, height, rgb,
                                                  d_dst, dst_pitch, dst_image_pitch),
                                    channels, pick_stream(h, stream)));
}

orbx_status orbx_cvt_gray(const uint8_t* src, size_t src_pitch, size_t src_image_pitch, int n_images, int width,
                          int height, int channels, int rgb, uint8_t* dst, size_t dst_pitch, size_t dst_image_pitch,
                          int device) {
  const orbx_status s =
      cvt_gray_check(src, src_pitch, src_image_pitch, n_images, width, height, channels, dst, dst_pitch, dst_image_pitch);
  if (s != ORBX_OK || n_images == 0 || width == 0 || height == 0) return s;
  const orbx_status dv = orbx::select_device(device);
  if (dv != ORBX_OK) return dv;
  // rows packed back to back on both sides of PCIe: the caller's padding is neither read nor written
  using orbx::Staging;
  const size_t srow = (size_t)channels * width, drow = (size_t)width;
  Staging S(device);
  const auto s_src = S.in<uint8_t>(nullptr, srow * height * n_images);
  const auto s_dst = S.out<uint8_t>(drow * height * n_images);
  const orbx_status cs = S.commit();
  if (cs != ORBX_OK) return cs;
  for (int i = 0; i < n_images; i++)
    pack_rows(S.host(s_src) + (size_t)i * height * srow, src + (size_t)i * src_image_pitch, src_pitch, srow, height);
  hipError_t e = S.upload(Staging::Outputs::skipped);
  if (e == hipSuccess)
    e = launch_cvt_gray(cvt_gray_args(S.dev(s_src), srow, srow * height, n_images, width, height, rgb, S.dev(s_dst), drow,
                                      drow * height),
                        channels, S.stream());
  if (e == hipSuccess) e = S.download();
  if (e == hipSuccess) e = S.sync();
  if (e != hipSuccess) return ORBX_ERR_HIP;
  for (int i = 0; i < n_images; i++)
    for (int y = 0; y < height; y++)
      std::memcpy(dst + (size_t)i * dst_image_pitch + (size_t)y * dst_pitch, S.host(s_dst) + ((size_t)i * height + y) * drow,
                  drow);
  return ORBX_OK;
}

orbx_status orbx_frame_rgbd(orbx_extractor* h, const uint8_t* img, size_t stride, int width, int height,
                            int channels, int rgb, const void* depth, size_t depth_stride, int depth_width,
                            int depth_height, int depth_type, float depth_factor, const orbx_camera* cam, float bf,
                            orbx_keypoint* kps, uint8_t* desc, int cap, int* n, orbx_keypoint* kps_un,
                            float* uRight, float* depth_out) {
  if (!h || !n) return ORBX_ERR_ARG;
  *n = 0;
  if (!img || width <= 0 || height <= 0) return ORBX_OK;  // src/ORBextractor.cc:1141, src/Frame.cc:147-148
  const size_t es = depth_elem(depth_type);
  if ((channels != 1 && channels != 3 && channels != 4) || es == 0 || !cam || !camera_ok(*cam)) return ORBX_ERR_ARG;
  if (!depth || depth_width != width || depth_height != height) return ORBX_ERR_ARG;
  const size_t irow = (size_t)channels * width, drow = es * width;
  if (stride < irow || depth_stride < drow || depth_stride % es || (uintptr_t)depth % es) return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  DevPlan* P = nullptr;
  orbx_status s = get_plan(h, width, height, &P);
  if (s != ORBX_OK) return s;
  const int kc = P->G.max_kps;
  const size_t npx = (size_t)width * height;
  // upload block: image rows packed | depth rows packed.  Device output block: count, depth count,
  // out-of-image count | keypoints | undistorted keypoints | descriptors | uRight | depth -- one copy back
  const size_t i_dep = scratch_align(irow * height), i_end = i_dep + drow * height;
  BlockCursor blk;
  const size_t o_kps = blk.take<orbx_keypoint>(kc), o_un = blk.take<orbx_keypoint>(kc),
               o_desc = blk.take<uint8_t>((size_t)kc * 32), o_ur = blk.take<float>(kc), o_dep = blk.take<float>(kc),
               o_end = blk.end();
  hipError_t e = hipSuccess;
  auto chk = [&](hipError_t x) { if (x != hipSuccess) e = x; };
  chk(h->rgbd_in.ensure(i_end + kInSlack));
  if (channels > 1) chk(h->in.ensure(npx + kInSlack));
  chk(h->out.ensure(o_end));
  chk(h->hstage.ensure(std::max(i_end, o_end)));
  if (e != hipSuccess) return ORBX_ERR_HIP;
  hipStream_t st = h->stream;
  uint8_t* hs = h->hstage.p;
  pack_rows(hs, img, stride, irow, height);
  pack_rows(hs + i_dep, depth, depth_stride, drow, height);
  if (hipMemcpyAsync(h->rgbd_in.p, hs, i_end, hipMemcpyHostToDevice, st) != hipSuccess) return ORBX_ERR_HIP;
  const uint8_t* d_gray = h->rgbd_in.p;  // a grey input is level 0 as uploaded
  if (channels > 1) {
    if (launch_cvt_gray(cvt_gray_args(h->rgbd_in.p, irow, irow * height, 1, width, height, rgb, h->in.p, width, npx),
                        channels, st) != hipSuccess)
      return ORBX_ERR_HIP;
    d_gray = h->in.p;
  }
  int32_t* d_counts = (int32_t*)h->out.p;
  orbx_keypoint* d_kps = (orbx_keypoint*)(h->out.p + o_kps);
  uint8_t* d_desc = h->out.p + o_desc;
  s = run_extract(h, P, 1, d_gray, npx, d_kps, d_desc, d_counts, kc, st);
  if (s != ORBX_OK) return s;
  s = run_rgbd_finish(1, d_kps, d_counts, kc, kc, *cam, bf,
                      {h->rgbd_in.p + i_dep, drow, drow * height, depth_type, width, height, depth_factor},
                      {(orbx_keypoint*)(h->out.p + o_un), (float*)(h->out.p + o_ur), (float*)(h->out.p + o_dep),
                       d_counts + 1, d_counts + 2},
                      st);
  if (s != ORBX_OK) return s;
  chk(hipMemcpyAsync(hs, h->out.p, o_end, hipMemcpyDeviceToHost, st));
  chk(hipStreamSynchronize(st));
  if (e != hipSuccess) return ORBX_ERR_HIP;
  const int32_t cnt = ((const int32_t*)hs)[0], oob = ((const int32_t*)hs)[2];
  *n = cnt;
  if (cnt > cap) return ORBX_ERR_CAPACITY;
  copy_out(kps, hs + o_kps, sizeof(orbx_keypoint) * cnt);
  copy_out(kps_un, hs + o_un, sizeof(orbx_keypoint) * cnt);
  copy_out(desc, hs + o_desc, (size_t)32 * cnt);
  copy_out(uRight, hs + o_ur, sizeof(float) * cnt);
  copy_out(depth_out, hs + o_dep, sizeof(float) * cnt);
  return oob != 0 ? ORBX_ERR_STATE : ORBX_OK;
}

orbx_status orbx_rgbd_frames_device(orbx_extractor* h, int n_frames, const uint8_t* d_images, int width, int height,
                                    int channels, int rgb, size_t row_pitch, size_t image_pitch, const void* d_depth,
                                    int depth_type, size_t depth_row_pitch, size_t depth_image_pitch,
                                    float depth_factor, const orbx_camera* cam, float bf, orbx_keypoint* d_kps,
                                    uint8_t* d_desc, int32_t* d_counts, int kp_capacity, orbx_keypoint* d_kps_un,
                                    float* d_uright, float* d_depth_out, int32_t* d_nmatches, void* stream) {
  if (!h || n_frames < 0 || !d_kps || !d_desc || !d_counts || !d_kps_un || !d_uright || !d_depth_out || !d_nmatches)
    return ORBX_ERR_ARG;
  if (n_frames == 0) return ORBX_OK;
  const size_t es = depth_elem(depth_type);
  if ((channels != 1 && channels != 3 && channels != 4) || es == 0 || !cam || !camera_ok(*cam)) return ORBX_ERR_ARG;
  if (!d_images || !d_depth || width <= 0 || height <= 0) return ORBX_ERR_ARG;
  const size_t irow = (size_t)channels * width, drow = es * width, npx = (size_t)width * height;
  if (row_pitch < irow || (channels == 1 && row_pitch != irow) || image_pitch < span_bytes(irow, row_pitch, height, 0, 1))
    return ORBX_ERR_ARG;
  if (depth_row_pitch < drow || depth_row_pitch % es || depth_image_pitch % es || (uintptr_t)d_depth % es ||
      depth_image_pitch < span_bytes(drow, depth_row_pitch, height, 0, 1))
    return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  hipStream_t st = pick_stream(h, stream);
  const uint8_t* d_gray = d_images;
  size_t gray_pitch = image_pitch;
  if (channels > 1) {
    const orbx_status cs = cvt_gray_check(d_images, row_pitch, image_pitch, n_frames, width, height, channels, d_images, width, npx);
    if (cs != ORBX_OK) return cs;
    if (h->in.ensure(npx * n_frames + kInSlack) != hipSuccess) return ORBX_ERR_HIP;
    if (launch_cvt_gray(cvt_gray_args(d_images, row_pitch, image_pitch, n_frames, width, height, rgb, h->in.p, width, npx),
                        channels, st) != hipSuccess)
      return ORBX_ERR_HIP;
    d_gray = h->in.p;
    gray_pitch = npx;
  }
  if (h->rgbd_oob.ensure((size_t)n_frames) != hipSuccess) return ORBX_ERR_HIP;
  orbx_status s = orbx_extract_batch_device(h, n_frames, d_gray, width, height, gray_pitch, d_kps, d_desc, d_counts,
                                            kp_capacity, stream);
  if (s != ORBX_OK) return s;
  return run_rgbd_finish(n_frames, d_kps, d_counts, kp_capacity, h->last_plan->G.max_kps, *cam, bf,
                         {(const uint8_t*)d_depth, depth_row_pitch, depth_image_pitch, depth_type, width, height, depth_factor},
                         {d_kps_un, d_uright, d_depth_out, d_nmatches, h->rgbd_oob.p}, st);
}

orbx_status orbx_profile_enable(orbx_extractor* h, int enable) {
  if (!h) return ORBX_ERR_ARG;
  h->timer.flush();
  h->timer.enabled = enable != 0;
  return ORBX_OK;
}

orbx_status orbx_profile_reset(orbx_extractor* h) {
  if (!h) return ORBX_ERR_ARG;
  (void)hipSetDevice(h->device);
  h->timer.reset();
  return ORBX_OK;
}

int orbx_profile_read(orbx_extractor* h, int stage, double* total_ms, long long* launches, const char** name) {
  if (!h) return ORBX_ERR_ARG;
  if (stage < 0) return ST_COUNT;
  if (stage >= ST_COUNT) return ORBX_ERR_ARG;
  (void)hipSetDevice(h->device);
  h->timer.flush();
  if (total_ms) *total_ms = h->timer.total_ms[stage];
  if (launches) *launches = h->timer.launches[stage];
  if (name) *name = kStageNames[stage];
  return ORBX_OK;
}

orbx_status orbx_descriptor_distance_device(const uint8_t* d_a, const uint8_t* d_b, int n, int32_t* d_out,
                                            void* stream) {
  if (n < 0 || (n > 0 && (!d_a || !d_b || !d_out))) return ORBX_ERR_ARG;
  return hip_status(launch_hamming(d_a, d_b, n, d_out, (hipStream_t)stream));
}

}  // extern "C"


// debug.hip -- the extractor's part of include/orbx_debug.h (tests and tools only): stage buffers of a
// handle's last extraction, the plan's launch descriptors built on the host, the stereo matcher on
// supplied keypoints, k_octree on supplied candidates, and the HBM copy reference of the roofline (this
// unit's one kernel).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/orbx_debug.h"
#include "orbx_extractor.h"

using namespace orbx;

extern "C" long long orbx_debug_copy(orbx_extractor* h, int what, int image, int arg, void* dst, size_t cap) {
  if (!h) return ORBX_ERR_ARG;
  if (!h->last_plan) return ORBX_ERR_STATE;
  const DevPlan& P = *h->last_plan;
  const Geometry& G = P.G;
  if (image < 0 || image >= h->last_n) return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return ORBX_ERR_HIP;
  std::vector<int> host;
  const void* src = nullptr;
  size_t bytes = 0;
  bool device_src = true;
  switch (what) {
    case ORBX_DBG_BLUR_LEVEL: {
      if (arg < 0 || arg >= G.nlevels) return ORBX_ERR_ARG;
      const LevelGeom& L = G.lv[arg];
      bytes = (size_t)L.w * L.h;
      if (dst && cap >= bytes) {
        // the blurred levels of the last batch, re-blurred from its pyramid (the same bytes k_blur
        // wrote; the batch that follows may have reused the buffer)
        if (h->blur.ensure((size_t)G.blur_bytes * h->last_n + 256) != hipSuccess) return ORBX_ERR_HIP;
        const BatchPtrs B = batch_ptrs(h, h->last_in, h->last_pitch);
        if (launch_blur(G, P.dG.p, P.dtiles.p, B, h->last_n, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess)
          return ORBX_ERR_HIP;
        const uint8_t* b = h->blur.p + (size_t)image * G.blur_bytes + L.boff;
        std::vector<uint8_t> tiles((size_t)L.bstride * ((L.h + 7) & ~7));
        if (hipMemcpy(tiles.data(), b, tiles.size(), hipMemcpyDeviceToHost) != hipSuccess) return ORBX_ERR_HIP;
        uint8_t* o = static_cast<uint8_t*>(dst);
        for (int yy = 0; yy < L.h; yy++)
          for (int xx = 0; xx < L.w; xx++)
            o[(size_t)yy * L.w + xx] = tiles[((size_t)(yy >> 3) * (L.bstride >> 4) + (xx >> 4)) * 128 + (yy & 7) * 16 + (xx & 15)];
      }
      return (long long)bytes;
    }
    case ORBX_DBG_CELL_COUNTS:
      src = h->cell_count.p + (size_t)image * G.ncells;
      bytes = sizeof(int) * G.ncells;
      break;
    case ORBX_DBG_CELL_TABLE: {  // cand_off: the cell's slot range in ORBX_DBG_CANDIDATES' view
      int loff = 0;
      for (const CellInfo& c : P.cells) {
        int v[8] = {c.level, c.x0, c.y0, c.x1, c.y1, loff, c.cap, 0};
        host.insert(host.end(), v, v + 8);
        loff += c.cap;
      }
      device_src = false;
      break;
    }
    case ORBX_DBG_CANDIDATES: {  // every cell's slots contiguous (inline then overflow), cells in order
      std::vector<uint32_t> raw((size_t)G.cand_total);
      if (hipMemcpy(raw.data(), h->cand.p + (size_t)image * G.cand_total, raw.size() * 4, hipMemcpyDeviceToHost) !=
          hipSuccess)
        return ORBX_ERR_HIP;
      std::vector<uint32_t> logical;
      logical.reserve(raw.size());
      for (const CellInfo& c : P.cells)
        for (int q = 0; q < c.cap; q++) logical.push_back(raw[cell_slot(c, q)]);
      static_assert(sizeof(uint32_t) == sizeof(int), "host staging is int words");
      host.resize(logical.size());
      std::memcpy(host.data(), logical.data(), logical.size() * 4);
      device_src = false;
      break;
    }
    case ORBX_DBG_OCT_COUNTS:
      src = h->oct_count.p + (size_t)image * G.nlevels;
      bytes = sizeof(int) * G.nlevels;
      break;
    case ORBX_DBG_OCT_OUT:
      src = h->oct.p + (size_t)image * G.oct_total;
      bytes = sizeof(uint32_t) * G.oct_total;
      break;
    case ORBX_DBG_LEVEL_INFO:
      for (int l = 0; l < G.nlevels; l++) {
        const LevelGeom& L = G.lv[l];
        int v[8] = {L.w, L.h, L.cell_begin, L.cell_end, L.oct_off, L.oct_cap, L.nfeat, L.nIni};
        host.insert(host.end(), v, v + 8);
      }
      device_src = false;
      break;
    case ORBX_DBG_PATCH_SLOTS:
      host.assign(patch_slot_table(), patch_slot_table() + 128);
      device_src = false;
      break;
    default:
      return ORBX_ERR_ARG;
  }
  if (!device_src) {
    bytes = host.size() * sizeof(int);
    if (dst) std::memcpy(dst, host.data(), std::min(bytes, cap));
    return (long long)bytes;
  }
  if (dst && cap) {
    if (hipMemcpy(dst, src, std::min(bytes, cap), hipMemcpyDeviceToHost) != hipSuccess) return ORBX_ERR_HIP;
  }
  return (long long)bytes;
}

// ------------------------------------------------------------ stereo matcher on supplied keypoints
// orbx_debug_stereo_keypoints_check: what k_stereo_prep / k_stereo_match index unguarded with a
// keypoint -- G->lv[octave], inv_scale[octave], the row table at (int)y -- and what their (octave, y)
// sort key assumes (y's float bits ordered as its value: no sign bit).  Host only.
extern "C" int orbx_debug_stereo_keypoints_check(const orbx_keypoint* kps, int n, int nlevels, int width,
                                                 int height) {
  if (n < 0 || (n > 0 && !kps) || nlevels < 1 || nlevels > kMaxLevelsPlan || width <= 0 || height <= 0)
    return ORBX_ERR_ARG;
  for (int i = 0; i < n; i++) {
    const orbx_keypoint& k = kps[i];
    if (k.octave < 0 || k.octave >= nlevels) return ORBX_ERR_ARG;
    if (!std::isfinite(k.x) || !std::isfinite(k.y) || std::signbit(k.x) || std::signbit(k.y)) return ORBX_ERR_ARG;
    if (!(k.x < (float)width) || !(k.y < (float)height)) return ORBX_ERR_ARG;
  }
  return ORBX_OK;
}

extern "C" orbx_status orbx_debug_stereo_keypoints(orbx_extractor* left, orbx_extractor* right,
                                                   const orbx_keypoint* kpsL, const uint8_t* descL, int nL,
                                                   const orbx_keypoint* kpsR, const uint8_t* descR, int nR, float bf,
                                                   float baseline, float* uRight, float* depth, int32_t* sad,
                                                   int32_t* nmatches) {
  if (!uRight || !depth || !sad || !nmatches || nL < 0 || nR < 0) return ORBX_ERR_ARG;
  if ((nL > 0 && (!kpsL || !descL)) || (nR > 0 && (!kpsR || !descR))) return ORBX_ERR_ARG;
  if (nR > kMaxStereoKps) return ORBX_ERR_CAPACITY;
  if (!left || !right) return ORBX_ERR_ARG;
  if (!left->last_plan || !right->last_plan || !left->last_host || !right->last_host) return ORBX_ERR_STATE;
  const Geometry& G = left->last_plan->G;
  if (G.width != right->last_plan->G.width || G.height != right->last_plan->G.height ||
      G.nlevels != right->last_plan->G.nlevels || left->device != right->device)
    return ORBX_ERR_ARG;
  if (orbx_debug_stereo_keypoints_check(kpsL, nL, G.nlevels, G.width, G.height) != ORBX_OK ||
      orbx_debug_stereo_keypoints_check(kpsR, nR, G.nlevels, G.width, G.height) != ORBX_OK)
    return ORBX_ERR_ARG;
  *nmatches = 0;
  if (nL == 0) return ORBX_OK;
  orbx_extractor* h = left;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  // scratch block of this call alone (the handles' output blocks keep their extractions):
  // counts (L, R) and the match count | keypoints L | R | descriptors L | R | uRight | depth
  BlockCursor cur;
  const size_t o_kL = cur.take<orbx_keypoint>(nL), o_kR = cur.take<orbx_keypoint>(nR),
               o_dL = cur.take<uint8_t>((size_t)nL * 32), o_dR = cur.take<uint8_t>((size_t)nR * 32),
               o_res = cur.take<float>((size_t)2 * nL);
  DevBuf<uint8_t> blk;
  if (blk.ensure(cur.end()) != hipSuccess) return ORBX_ERR_HIP;
  hipError_t e = hipSuccess;
  auto chk = [&](hipError_t x) { if (x != hipSuccess) e = x; };
  hipStream_t st = h->stream;
  const int32_t counts[3] = {nL, nR, 0};
  chk(hipMemcpyAsync(blk.p, counts, sizeof(counts), hipMemcpyHostToDevice, st));
  chk(hipMemcpyAsync(blk.p + o_kL, kpsL, (size_t)nL * sizeof(orbx_keypoint), hipMemcpyHostToDevice, st));
  chk(hipMemcpyAsync(blk.p + o_dL, descL, (size_t)nL * 32, hipMemcpyHostToDevice, st));
  if (nR > 0) {
    chk(hipMemcpyAsync(blk.p + o_kR, kpsR, (size_t)nR * sizeof(orbx_keypoint), hipMemcpyHostToDevice, st));
    chk(hipMemcpyAsync(blk.p + o_dR, descR, (size_t)nR * 32, hipMemcpyHostToDevice, st));
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    return ORBX_ERR_HIP;
  }
  int32_t* d_counts = (int32_t*)blk.p;
  float* d_ur = (float*)(blk.p + o_res);
  // the shipped launch path, as orbx_stereo_match takes it (the pyramids are the handles' own)
  const StereoSides S = StereoSides::handles((const orbx_keypoint*)(blk.p + o_kL), blk.p + o_dL, d_counts,
                                             (const orbx_keypoint*)(blk.p + o_kR), blk.p + o_dR, d_counts + 1);
  orbx_status s = run_stereo(left, right, 1, S, nL, bf, baseline, d_ur, d_ur + nL, nL, d_counts + 2, st);
  if (s == ORBX_OK) {
    chk(hipMemcpyAsync(uRight, d_ur, sizeof(float) * nL, hipMemcpyDeviceToHost, st));
    chk(hipMemcpyAsync(depth, d_ur + nL, sizeof(float) * nL, hipMemcpyDeviceToHost, st));
    chk(hipMemcpyAsync(sad, h->sad.p, sizeof(int32_t) * nL, hipMemcpyDeviceToHost, st));
    chk(hipMemcpyAsync(nmatches, d_counts + 2, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  chk(hipStreamSynchronize(st));  // before blk is freed
  if (s != ORBX_OK) return s;
  return hip_status(e);
}

// ------------------------------------------------------------ k_octree on supplied candidates
// What k_octree reads of a candidate unguarded: put_cand subtracts the level's minBX / minBY and packs
// 12-bit fields, a cell's count indexes its slots up to cap, and the best-response pass assumes one
// candidate per pixel (FAST's non-maximum suppression never emits two).  counts: n_img x ncells;
// cand: n_img x (sum of the cells' caps), a cell's survivors from its logical offset on.  Host only.
constexpr int kOctInjectMaxImages = 64;
static bool octree_candidates_ok(const Plan& P, int n_img, const int32_t* counts, const uint32_t* cand) {
  const Geometry& G = P.G;
  if (n_img < 1 || n_img > kOctInjectMaxImages || !counts || !cand || G.ncells < 1) return false;
  long long total = 0;
  for (const CellInfo& c : P.cells) total += c.cap;
  std::vector<uint8_t> seen;
  for (int img = 0; img < n_img; img++) {
    const int32_t* cnt = counts + (size_t)img * G.ncells;
    const uint32_t* cd = cand + (size_t)img * total;
    for (int l = 0; l < G.nlevels; l++) {
      const LevelGeom& L = G.lv[l];
      seen.assign((size_t)L.w * L.h, 0);
      for (int ci = L.cell_begin; ci < L.cell_end; ci++) {
        if (cnt[ci] < 0 || cnt[ci] > P.cells[ci].cap) return false;
        for (int q = 0; q < cnt[ci]; q++) {
          const uint32_t v = cd[q];
          const int x = (int)(v & 0xFFF), y = (int)((v >> 12) & 0xFFF);
          if (x < L.minBX || x >= L.maxBX || y < L.minBY || y >= L.maxBY) return false;
          uint8_t& s = seen[(size_t)y * L.w + x];
          if (s) return false;
          s = 1;
        }
        cd += P.cells[ci].cap;
      }
    }
  }
  return true;
}

extern "C" int orbx_debug_octree_candidates_check(const orbx_extractor_params* params, int width, int height,
                                                  int n_img, const int32_t* cell_counts, const uint32_t* candidates) {
  if (!params_ok(params) || width <= 0 || height <= 0) return ORBX_ERR_ARG;
  Plan P;
  const orbx_status s = build_plan(*params, make_tables(*params), width, height, P);
  if (s != ORBX_OK) return s;
  return octree_candidates_ok(P, n_img, cell_counts, candidates) ? ORBX_OK : ORBX_ERR_ARG;
}

// paths (n_img x nlevels, or null) and depth_cap: launch_octree's
static orbx_status octree_candidates_run(orbx_extractor* h, int n_img, const int32_t* cell_counts,
                                         const uint32_t* candidates, int32_t* oct_count, uint32_t* oct_out,
                                         int32_t* paths, int depth_cap) {
  if (!h || !oct_count || !oct_out) return ORBX_ERR_ARG;
  if (!h->last_plan) return ORBX_ERR_STATE;
  const DevPlan& P = *h->last_plan;
  const Geometry& G = P.G;
  if (!octree_candidates_ok(P, n_img, cell_counts, candidates)) return ORBX_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return ORBX_ERR_HIP;
  // scratch block of this call alone (the handle's batch buffers keep their extraction):
  // candidates in cell_slot's layout | cell counts | k_octree's spill scratch (positions, nodes) |
  // output slots | output counts
  const size_t n = (size_t)n_img;
  BlockCursor cur;
  const size_t o_cand = cur.take<uint32_t>(n * G.cand_total), o_cnt = cur.take<int>(n * G.ncells),
               o_kpos = cur.take<uint32_t>(n * G.cand_total), o_knode = cur.take<int>(n * G.cand_total),
               o_oct = cur.take<uint32_t>(n * G.oct_total), o_octn = cur.take<int>(n * G.nlevels),
               o_path = cur.take<int>(n * G.nlevels);
  DevBuf<uint8_t> blk;
  if (blk.ensure(cur.end()) != hipSuccess) return ORBX_ERR_HIP;
  std::vector<uint32_t> raw(n * G.cand_total, 0);
  {
    const uint32_t* cd = candidates;
    for (int img = 0; img < n_img; img++)
      for (int ci = 0; ci < G.ncells; ci++) {
        const CellInfo& c = P.cells[ci];
        for (int q = 0; q < cell_counts[(size_t)img * G.ncells + ci]; q++)
          raw[(size_t)img * G.cand_total + cell_slot(c, q)] = cd[q];
        cd += c.cap;
      }
  }
  hipError_t e = hipSuccess;
  auto chk = [&](hipError_t x) { if (x != hipSuccess) e = x; };
  hipStream_t st = h->stream;
  chk(hipMemcpyAsync(blk.p + o_cand, raw.data(), raw.size() * 4, hipMemcpyHostToDevice, st));
  chk(hipMemcpyAsync(blk.p + o_cnt, cell_counts, n * G.ncells * sizeof(int), hipMemcpyHostToDevice, st));
  chk(hipMemsetAsync(blk.p + o_oct, 0xFF, n * G.oct_total * 4, st));
  chk(hipMemsetAsync(blk.p + o_octn, 0xFF, n * G.nlevels * sizeof(int), st));
  chk(hipMemsetAsync(blk.p + o_path, 0xFF, n * G.nlevels * sizeof(int), st));
  if (e == hipSuccess) {
    BatchPtrs B{};
    B.cand = (uint32_t*)(blk.p + o_cand);
    B.cell_count = (int*)(blk.p + o_cnt);
    B.kpos = (uint32_t*)(blk.p + o_kpos);
    B.knode = (int*)(blk.p + o_knode);
    B.oct = (uint32_t*)(blk.p + o_oct);
    B.oct_count = (int*)(blk.p + o_octn);
    // the dynamic LDS limit is per kernel, not per plan: another geometry's plan may have set it since
    size_t mx = octree_group_smem(G.og_all);
    for (int g = 0; g < G.n_og; g++) mx = std::max(mx, octree_group_smem(G.og[g]));
    chk(octree_set_smem_limit(mx));
    // the shipped launch path, as launch_extract_stages takes it (which passes no path pointer and no cap)
    if (e == hipSuccess)
      chk(launch_octree(G, P.dG.p, P.dcells.p, B, n_img, st, paths ? (int*)(blk.p + o_path) : nullptr, depth_cap));
  }
  if (e == hipSuccess && paths)
    chk(hipMemcpyAsync(paths, blk.p + o_path, n * G.nlevels * sizeof(int), hipMemcpyDeviceToHost, st));
  if (e == hipSuccess) {
    chk(hipMemcpyAsync(oct_count, blk.p + o_octn, n * G.nlevels * sizeof(int), hipMemcpyDeviceToHost, st));
    chk(hipMemcpyAsync(oct_out, blk.p + o_oct, n * G.oct_total * 4, hipMemcpyDeviceToHost, st));
  }
  chk(hipStreamSynchronize(st));  // before blk is freed
  return hip_status(e);
}

extern "C" orbx_status orbx_debug_octree_candidates(orbx_extractor* h, int n_img, const int32_t* cell_counts,
                                                    const uint32_t* candidates, int32_t* oct_count,
                                                    uint32_t* oct_out) {
  return octree_candidates_run(h, n_img, cell_counts, candidates, oct_count, oct_out, nullptr, -1);
}

extern "C" orbx_status orbx_debug_octree_paths(orbx_extractor* h, int n_img, const int32_t* cell_counts,
                                               const uint32_t* candidates, int depth_cap, int32_t* oct_count,
                                               uint32_t* oct_out, int32_t* paths) {
  if (!paths || depth_cap < -1) return ORBX_ERR_ARG;
  return octree_candidates_run(h, n_img, cell_counts, candidates, oct_count, oct_out, paths, depth_cap);
}

extern "C" long long orbx_debug_launch_plan(const orbx_extractor_params* params, int width, int height, int what,
                                            int a0, int a1, int a2, long long* dst, size_t cap) {
  std::vector<long long> out;
  auto done = [&]() {
    if (dst) std::memcpy(dst, out.data(), std::min(out.size(), cap) * sizeof(long long));
    return (long long)out.size();
  };
  if (what == ORBX_LP_REMAP) {
    XcdRemap R{};
    if (a0 < 1 || a1 < 1 || a2 < 1 || !make_xcd_remap((unsigned)a0, (unsigned)a1, (unsigned)a2, &R)) return ORBX_ERR_ARG;
    out = {R.gx, R.gy, R.q, R.r, R.mx, R.sx, R.my, R.sy};
    return done();
  }
  if (!params_ok(params) || width <= 0 || height <= 0) return ORBX_ERR_ARG;
  Plan P;
  const orbx_status s = build_plan(*params, make_tables(*params), width, height, P);
  if (s != ORBX_OK) return s;
  // the descriptors over the host tables: a pointer's element offset is its distance from the base
  LaunchPlan LP;
  build_launch_plan(P, P.xt.data(), P.yt.data(), P.rzb.data(), LP);
  const Geometry& G = P.G;
  switch (what) {
    case ORBX_LP_LEVELS:
      for (int l = 0; l < G.nlevels; l++) {
        const LevelGeom& L = G.lv[l];
        out.insert(out.end(), {L.w, L.h, L.off, L.boff, L.bstride, L.tile_begin, L.tiles_x, L.tiles_y});
      }
      break;
    case ORBX_LP_RESIZE:
      for (int l = 1; l < G.nlevels; l++) {
        const ResizeDesc& D = LP.rz[l];
        out.insert(out.end(), {D.sw, D.sh, D.dw, D.dh, D.src_off, D.dst_off, D.pyr_bytes, D.X - P.xt.data(),
                               D.Y - P.yt.data(), D.bx - P.rzb.data(), D.by - P.rzb.data(), D.stride, D.rows, D.lc,
                               (D.dw + kRzTW - 1) / kRzTW, (D.dh + kRzTH - 1) / kRzTH});
      }
      break;
    case ORBX_LP_BOUNDS:
      for (int i = 0; i < P.rzb_n; i++) out.insert(out.end(), {P.rzb[i].x, P.rzb[i].y});
      break;
    case ORBX_LP_PATH:
      for (int l = 1; l < G.nlevels; l++) {
        const bool f = P.strip[l];
        const int tw = f ? kRsTW : kRzTW, th = f ? kRsTH : kRzTH;
        out.insert(out.end(), {f ? 1 : 0, (G.lv[l].w + tw - 1) / tw, (G.lv[l].h + th - 1) / th, tw, th,
                               f ? kRsStride : G.rz_stride, f ? kRsRows : G.rz_rows, f ? kRsR : 0});
      }
      break;
    case ORBX_LP_FAST:
      for (int g = 0; g < G.n_fg; g++) {
        const Geometry::FastGroup& F = G.fg[g];
        out.insert(out.end(), {F.c0, F.c1, F.s, F.rp, F.nk, F.tile_bytes, F.map_bytes, F.smem});
      }
      break;
    case ORBX_LP_OCTREE: {
      auto row = [&](const OctGroup& g, long long max_batch) {
        out.insert(out.end(), {g.l0, g.l1, g.nt, g.node_cap, g.cell_cap, g.kcap,
                               (long long)octree_group_smem(g), max_batch});
      };
      for (int g = 0; g < G.n_og; g++) row(G.og[g], -1);
      row(G.og_all, kOctOneLaunch);
      break;
    }
    case ORBX_LP_OCT_PYRAMID: {
      auto row = [&](const OctGroup& g) {
        const long long n = g.depth > 0 ? oct_pyr_counters(g.nini, g.depth) : 0;
        out.insert(out.end(), {g.depth, g.nini, n, (n + 1) / 2 * 4,
                               g.depth > 0 ? (long long)oct_pyr_layout(g.node_cap, g.cell_cap, g.pcap, g.span, g.nini, g.depth).bytes : 0,
                               (long long)octree_smem_bytes(g.node_cap, g.cell_cap, g.kcap),
                               (long long)octree_group_smem(g), kOctMaxDepth});
      };
      for (int g = 0; g < G.n_og; g++) row(G.og[g]);
      row(G.og_all);
      break;
    }
    case ORBX_LP_CELLS: {
      long long loff = 0;
      for (const CellInfo& c : P.cells) {
        out.insert(out.end(), {c.level, c.x0, c.y0, c.x1, c.y1, loff, c.cap, c.kin});
        loff += c.cap;
      }
      break;
    }
    case ORBX_LP_OCT_LEVELS:
      for (int l = 0; l < G.nlevels; l++) {
        const LevelGeom& L = G.lv[l];
        out.insert(out.end(), {L.minBX, L.minBY, L.maxBX, L.maxBY, L.nfeat, L.nIni, L.oct_off, L.oct_cap});
      }
      break;
    case ORBX_LP_GRIDS: {
      if (a0 < 1) return ORBX_ERR_ARG;
      for (int l = 1; l < G.nlevels; l++)
        out.insert(out.end(), {(G.lv[l].w + kRzTW - 1) / kRzTW, (G.lv[l].h + kRzTH - 1) / kRzTH, a0});
      out.insert(out.end(), {G.ntiles, a0, 1});
      break;
    }
    case ORBX_LP_XTAB:
    case ORBX_LP_YTAB: {
      if (a0 < 1 || a0 >= G.nlevels) return ORBX_ERR_ARG;
      const LevelGeom& L = G.lv[a0];
      if (what == ORBX_LP_XTAB)
        for (int i = 0; i < L.w; i++) {
          const ResizeX& X = P.xt[L.xtab_off + i];
          out.insert(out.end(), {X.sx0, X.sx1, X.a0, X.a1});
        }
      else
        for (int i = 0; i < L.h; i++) {
          const ResizeY& Y = P.yt[L.ytab_off + i];
          out.insert(out.end(), {Y.sy0, Y.sy1, Y.b0, Y.b1});
        }
      break;
    }
    default:
      return ORBX_ERR_ARG;
  }
  return done();
}

// On-box HBM reference for the roofline: a streaming device-to-device copy,
// one 16-B non-temporal load + store per thread over the whole buffer (the
// fastest of the forms measured: 6.52 TB/s against 6.21 with default-policy
// accesses and 4.7-5.0 with grid-stride loops).  *ms = mean time per copy.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_hbm_copy(u32x4* __restrict__ dst, const u32x4* __restrict__ src, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}

extern "C" int orbx_debug_hbm_copy(void* dst, const void* src, size_t bytes, int reps, float* ms) {
  if (!dst || !src || (bytes & 15) || reps < 1 || bytes / 16 / 256 >= (size_t)1 << 31) return ORBX_ERR_ARG;
  const size_t n = bytes / 16;
  const int grid = (int)((n + 255) / 256);
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess) return ORBX_ERR_HIP;
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    return ORBX_ERR_HIP;
  }
  hipLaunchKernelGGL(k_hbm_copy, dim3(grid), dim3(256), 0, 0, (u32x4*)dst, (const u32x4*)src, n);  // warm-up
  (void)hipEventRecord(e0, 0);
  for (int r = 0; r < reps; r++)
    hipLaunchKernelGGL(k_hbm_copy, dim3(grid), dim3(256), 0, 0, (u32x4*)dst, (const u32x4*)src, n);
  (void)hipEventRecord(e1, 0);
  hipError_t e = hipEventSynchronize(e1);
  float t = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (e != hipSuccess) return ORBX_ERR_HIP;
  if (ms) *ms = t / reps;
  return ORBX_OK;
}

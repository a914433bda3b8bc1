// orbx_internal.h -- geometry "plan" of one (width, height, params) extractor
// configuration, laid out for the device, plus kernel launch entry points.
//
// HBM layout per image (all u8, row-major, stride = level width):
//   level 0            : the caller's input image itself (never copied)
//   pyramid  (levels>=1): pyr  + img*pyr_bytes  + lv[l].off
//   blurred  (all levels): blur + img*blur_bytes + lv[l].boff, 8x16-byte tiles (128 B each),
//                          tile (ty, tx) at (ty * bstride/16 + tx) * 128, row y&7 at 16 * (y & 7)
//   FAST candidates     : cand + img*cand_total + cell_slot(cells[c], p) (u32 score<<24|y<<12|x): a cell's
//                          first kin survivors in its inline slots at cand_off, the rest at ovf_off
//   octree output       : oct  + img*oct_total  + lv[l].oct_off        (same packing, list order)
//
// Geometry is the plan as the kernels read it from device memory.  k_resize alone never touches it:
// what it needs comes by value in its launch descriptor (ResizeDesc, below).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbx.h"
#include "orbx_device.h"

namespace orbx {

constexpr int kMaxLevelsPlan = 16;
constexpr int kEdgeThresholdHost = 19;  // EDGE_THRESHOLD, src/ORBextractor.cc:74

struct LevelGeom {
  int w, h;
  long long off;    // offset of level in per-image pyramid buffer (levels >= 1)
  long long boff;   // offset of level in per-image blurred buffer (256-B aligned)
  int bstride;      // blurred level width rounded to 16 (tile columns = bstride / 16)
  int minBX, minBY, maxBX, maxBY;  // FAST border box, src/ORBextractor.cc:829-832
  int cell_begin, cell_end;        // range in the cell table (row-major)
  int cand_begin, cand_cap;        // candidate slots of the level in the per-image buffer
  int nfeat;                       // mnFeaturesPerLevel[l]
  int nIni;                        // octree root count, src/ORBextractor.cc:567
  float hX;                        // root width
  int oct_off, oct_cap;            // octree output slots
  float scale;                     // mvScaleFactor[l]
  float kp_size;                   // (float)(int)(PATCH_SIZE * scale)
  int xtab_off, ytab_off;          // resize tables (levels >= 1)
  int tile_begin, tiles_x, tiles_y;  // blur tiles
};

// batches up to this many images run k_octree as one launch over every level (Geometry::og_all)
constexpr int kOctOneLaunch = 2;
// k_octree launch group: levels [l0, l1) as NT-thread blocks with LDS sized for those levels
struct OctGroup {
  int l0, l1, nt;
  int node_cap;  // LDS node capacity (max over the group's levels, multiple of 64)
  int cell_cap;  // max cells of one level
  int kcap;      // candidates of a level kept in LDS (the rest in global scratch)
  int depth;     // count-pyramid depth D of the group's blocks (0: the generic path only)
  int nini;      // largest root count of the group's levels (sizes the pyramid)
  int span;      // largest border-box width + height of the group's levels (the pyramid path's column
                 // and row tables)
  int pcap;      // candidates the pyramid path keeps in LDS: kcap plus what the group's LDS has left
};

// k_octree's dynamic LDS for a launch group (OctSmem in extract.hip carves it up in this order); the
// plan sizes a group's kcap with it, the launch passes it
__host__ __device__ inline int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

__host__ __device__ inline size_t octree_smem_bytes(int NC, int cell_cap, int kcap) {
  const int NP2 = next_pow2(NC);
  size_t b = 0;
  b += 2 * 4 * NC * sizeof(int16_t);
  b += 2 * 2 * NC * sizeof(int);
  b += NC * 4 * sizeof(int);
  b += NC * 4 * sizeof(int16_t);
  b += NC * sizeof(int16_t);
  b += 2 * NC * sizeof(int);
  b = (b + 7) & ~(size_t)7;
  b += (size_t)NP2 * sizeof(uint64_t);
  b += (cell_cap + 1) * sizeof(int);
  b += 8 * sizeof(int);
  b += (size_t)kcap * (sizeof(uint32_t) + sizeof(uint16_t));
  return b;
}

// k_octree's count pyramid: one 16-bit counter per box of the fixed split geometry, depth d = 0 (the
// roots) .. D; box (d, gx, gy) has gx < nIni << d, gy < 1 << d and sits at oct_pyr_off(nIni, d) +
// gy * (nIni << d) + gx.  Depth 0 is padded to an even count, so the two children (2gx, 2gx + 1) of a
// row share one aligned dword.
constexpr int kOctMaxDepth = 6;
__host__ __device__ inline int oct_pyr_off(int nIni, int d) {
  return d == 0 ? 0 : ((nIni + 1) & ~1) + nIni * (((1 << (2 * d)) - 4) / 3);
}
__host__ __device__ inline int oct_pyr_counters(int nIni, int D) { return oct_pyr_off(nIni, D + 1); }

// LDS of k_octree's pyramid path (byte offsets into the block's dynamic LDS, which it shares with
// the generic path's OctSmem: a block runs one path at a time)
struct OctPyrLayout {
  int key, tmp, cell, cnt, seq, sa, sb, cpre, ctrl, kp, nidx, tab, pyr, bytes;
};
__host__ __device__ inline OctPyrLayout oct_pyr_layout(int NC, int cell_cap, int pcap, int span, int nIni, int D) {
  OctPyrLayout o;
  int b = 0;
  o.key = b;  b += next_pow2(NC) * 8;  // u64 [NP2]: packed scan words, sort keys, best responses
  o.tmp = b;  b += NC * 8;             // u64 [NC]: the rank sort's output
  o.cell = b; b += 2 * NC * 4;         // double-buffered node list: box d << 28 | gy << 20 | gx,
  o.cnt = b;  b += 2 * NC * 4;         //   candidates,
  o.seq = b;  b += 2 * NC * 4;         //   creation sequence
  o.sa = b;   b += NC * 4;
  o.sb = b;   b += NC * 4;
  o.cpre = b; b += (cell_cap + 1) * 4;
  o.ctrl = b; b += 8 * 4;
  o.kp = b;   b += pcap * 4;           // the level's first pcap candidates as read (score << 24 | y << 12 | x)
  o.pyr = b;  b += (oct_pyr_counters(nIni, D) + 1) / 2 * 4;
  o.nidx = b; b += NC * 2;
  o.tab = b;  b += span * 2;           // u16: column x -> gx at depth D, then row y -> gy
  o.bytes = (b + 3) & ~3;
  return o;
}

// dynamic LDS of a launch group's blocks.  The plan picks the group's depth so that the pyramid
// path fits in what the generic path takes: a group's LDS per block, and with it the blocks per CU,
// is what it was before the pyramid.
__host__ __device__ inline size_t octree_group_smem(const OctGroup& g) {
  const size_t a = octree_smem_bytes(g.node_cap, g.cell_cap, g.kcap);
  const size_t b = g.depth > 0 ? (size_t)oct_pyr_layout(g.node_cap, g.cell_cap, g.pcap, g.span, g.nini, g.depth).bytes : 0;
  return a > b ? a : b;
}

struct Geometry {
  int nlevels, width, height;
  int ini_th, min_th;
  LevelGeom lv[kMaxLevelsPlan];
  long long pyr_bytes, blur_bytes;
  int ncells, cand_total, oct_total, max_kps, ntiles;
  OctGroup og[2];  // k_octree launch groups (levels 0..split-1 at 512 threads, the rest at 256)
  int n_og;
  OctGroup og_all;  // every level in one launch (batches of <= kOctOneLaunch images)
  // k_fast launch groups (consecutive cell ranges, one launch each) with their LDS layout, sized by
  // the group's largest cell: row stride s of the window tile and the score map (40, 48 or 80),
  // region rows per compass instruction rp (2 when the group's cells are <= 32 wide)
  struct FastGroup {
    int c0, c1, s, rp, tile_bytes, map_bytes, smem;
    int nk;  // 16-B window loads per lane (k_fast's NK): covers the group's tallest window
  } fg[2];
  int n_fg;
  int rz_rows;    // k_resize: max source rows staged per 128x16 output tile
  int rz_stride;  // k_resize: LDS row stride of the staged footprint (16-B chunks covering the widest span)
  int rz_lc;      // k_resize: log2 of the lanes per footprint row (>= the widest span's 16-B chunks)
};

constexpr int kRzTW = 128, kRzTH = 32;  // k_resize output tile
constexpr int kRzMaxRows = 64;

// k_resize_strip (the fast path of a level, chosen at plan time: strip_resize_ok in plan.hip): a wave
// owns one strip of kRsR output rows across the 256-column tile (lane = 4 adjacent columns), a block
// four strips.  Footprint rows in LDS at a compile-time stride.
#ifndef ORBX_RS_R
#define ORBX_RS_R 8
#endif
constexpr int kRsR = ORBX_RS_R;
constexpr int kRsTW = 256, kRsTH = 4 * kRsR;  // output tile
constexpr int kRsStride = 336;                // LDS row stride: spans up to 256 columns x 1.25 (+ taps), 16-B chunks
constexpr int kRsRows = kRsTH * 5 / 4 + 3;    // footprint rows staged per tile

// A cell's FAST survivors: the first `kin` in its inline slots at cand_off (the cells' inline slots
// packed back to back, so the octree's per-cell reads share 128-B lines), the rest (up to `cap`) in
// its overflow slots at ovf_off.  Both offsets are per image within one cand_total block.
struct CellInfo {
  int16_t level, kin;
  int16_t x0, y0, x1, y1;  // FAST detection region (inclusive, level coordinates)
  int cand_off, cap;
  int lw, loff;  // the level's width and byte offset in an image's pyramid block (level > 0):
                 // k_fast finds its window from this one record, no dependent geometry load
  int ovf_off;
};
// slot p (< cap) of a cell's survivors, relative to the image's candidate block
__host__ __device__ inline int cell_slot(const CellInfo& c, int p) {
  return p < c.kin ? c.cand_off + p : c.ovf_off + (p - c.kin);
}

struct ResizeX {  // horizontal tap of one output column
  int sx0, sx1;
  int16_t a0, a1;
};
struct ResizeY {
  int sy0, sy1;
  int16_t b0, b1;
};

#ifndef ORBX_BLUR_TW  // k_blur output tile (256 threads: TW/4 column groups x 16-row strips)
#define ORBX_BLUR_TW 128
#define ORBX_BLUR_TH 128
#endif
constexpr int kBlurTileW = ORBX_BLUR_TW, kBlurTileH = ORBX_BLUR_TH;
static_assert(kBlurTileW / 4 * (kBlurTileH / 16) == 256, "k_blur: one thread per 4 columns x 16 rows");

// Device pointers for one batch.
struct BatchPtrs {
  const uint8_t* in;
  size_t in_pitch;
  uint8_t* pyr;
  uint8_t* blur;
  uint32_t* cand;
  int* cell_count;
  uint32_t* kpos;   // octree scratch
  int* knode;
  uint32_t* oct;
  int* oct_count;
};

__host__ __device__ inline const uint8_t* level_ptr(const Geometry& G, const BatchPtrs& B, int img, int l) {
  return l == 0 ? B.in + (size_t)img * B.in_pitch : B.pyr + (size_t)img * G.pyr_bytes + G.lv[l].off;
}

// ------------------------------------------------------------ launch descriptor
// Everything block-uniform that k_resize needs before its first pixel load, passed BY VALUE as a
// kernel argument: a block reads its kernel arguments, then its tile's footprint bounds (two pairs,
// one wait), then pixels -- two serial scalar-load waits where walking Geometry took seven, in a
// kernel whose waves live under 3,000 cycles.  Built once per plan on the host (build_launch_plan);
// only `rm` depends on the batch size and is filled at launch.  (k_blur and k_fast were given the
// same treatment and measured flat against the Geometry walk, profiles/r07/ab_descriptors_blur_fast.txt:
// their waves live 6,000-10,000 cycles.  They keep the walk.)
// One per level l >= 1 (source = level l - 1).
struct ResizeDesc {
  XcdRemap rm;
  int sw, sh, dw, dh;      // source and destination level sizes
  long long src_off;       // source level in an image's pyramid block; < 0: level 0, the input image
  long long dst_off;       // destination level in an image's pyramid block
  long long pyr_bytes;
  const ResizeX* X;        // the level's coefficient tables (xt + xtab_off, yt + ytab_off)
  const ResizeY* Y;
  const int2* bx;          // per tile column: (sx0 of its first, sx1 of its last output column)
  const int2* by;          // per tile row:    (sy0 of its first, sy1 of its last output row)
  int stride, rows, lc;    // Geometry::rz_stride, rz_rows, rz_lc
  int strip;               // 1: the level runs k_resize_strip, its tiles' bounds in sbx / sby; 0: k_resize
  const int2* sbx;         // per 256-column strip tile: (sx0 of its first, sx1 of its last output column)
  const int2* sby;         // per kRsTH-row strip tile:  (sy0 of its first, sy1 of its last output row)
#ifdef ORBX_RZ_PROBE
  int probe_base, level;   // the level's first block slot in the probe buffer (filled at launch)
#endif
};

struct LaunchPlan {
  ResizeDesc rz[kMaxLevelsPlan];  // [l], l >= 1
};

// ------------------------------------------------------------ extract.hip's host entry points
struct StageTimer;
hipError_t upload_constants(const int* umax16, const int* gauss7);
hipError_t launch_blur(const Geometry& Gh, const Geometry* Gd, const int* tile_level, const BatchPtrs& B, int n_img,
                       hipStream_t st);
// path (device, n_img x nlevels, or null): the path each block took, 0 empty level, 1 pyramid, 2 generic;
// depth_cap >= 0 lowers the groups' pyramid depth for this launch (the debug entry's; 0: generic only)
hipError_t launch_octree(const Geometry& Gh, const Geometry* Gd, const CellInfo* cells, const BatchPtrs& B, int n_img,
                         hipStream_t st, int* path = nullptr, int depth_cap = -1);
hipError_t launch_extract_stages(const Geometry& Gh, const Geometry* Gd, const CellInfo* cells, const int* tile_level,
                                 const LaunchPlan& LP, const BatchPtrs& B, int n_img, orbx_keypoint* kps, uint8_t* desc,
                                 int32_t* counts, int kp_cap, hipStream_t st, StageTimer* T);
hipError_t octree_set_smem_limit(size_t bytes);
const uint8_t* patch_slot_table();

}  // namespace orbx

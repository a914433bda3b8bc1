// plan.hip -- the per-geometry plan of the extraction kernels (orbx_plan.h): the reference
// constructor's tables, level sizes, FAST cell table and launch groups, octree launch groups, resize
// coefficient tables and the resize kernels' footprint bounds and launch descriptors.
//
// Host arithmetic only: this unit makes no HIP runtime call (it is a .hip for the vector types and
// the __host__ __device__ helpers of orbx_internal.h), so it also builds into a stand-alone test.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "orbx_plan.h"

namespace orbx {

static inline int round_even(float v) { return (int)std::nearbyintf(v); }

// ORBextractor::ORBextractor (src/ORBextractor.cc:416-490): scale factors in
// float from a double member, per-level quotas with cvRound, umax circle.
Tables make_tables(const orbx_extractor_params& p) {
  Tables t;
  const double sf = (double)p.scale_factor;
  const int n = p.nlevels;
  t.scale.assign(n, 1.0f);
  t.sigma2.assign(n, 1.0f);
  for (int i = 1; i < n; i++) {
    t.scale[i] = (float)((double)t.scale[i - 1] * sf);
    t.sigma2[i] = t.scale[i] * t.scale[i];
  }
  t.inv_scale.resize(n);
  t.inv_sigma2.resize(n);
  for (int i = 0; i < n; i++) {
    t.inv_scale[i] = 1.0f / t.scale[i];
    t.inv_sigma2[i] = 1.0f / t.sigma2[i];
  }
  t.nfeat.resize(n);
  const float factor = (float)(1.0f / sf);
  float ndes = (float)p.nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)n));
  int sum = 0;
  for (int l = 0; l < n - 1; l++) {
    t.nfeat[l] = round_even(ndes);
    sum += t.nfeat[l];
    ndes *= factor;
  }
  t.nfeat[n - 1] = std::max(p.nfeatures - sum, 0);
  int vmax = (int)std::floor(15 * std::sqrt(2.f) / 2 + 1);
  int vmin = (int)std::ceil(15 * std::sqrt(2.f) / 2);
  for (int v = 0; v < 16; v++) t.umax[v] = 0;
  for (int v = 0; v <= vmax; ++v) t.umax[v] = (int)std::nearbyint(std::sqrt(225.0 - v * v));
  for (int v = 15, v0 = 0; v >= vmin; --v) {
    while (t.umax[v0] == t.umax[v0 + 1]) ++v0;
    t.umax[v] = v0;
    ++v0;
  }
  return t;
}

// getGaussianKernel(7, 2, CV_32F) -> x256 -> cvRound (OpenCV 3.2 8U separable path).
void gaussian_int_kernel(int k[7]) {
  float cf[7];
  double sum = 0;
  const double scale2X = -0.5 / (2.0 * 2.0);
  for (int i = 0; i < 7; i++) {
    double x = i - 3.0;
    cf[i] = (float)std::exp(scale2X * x * x);
    sum += cf[i];
  }
  sum = 1. / sum;
  for (int i = 0; i < 7; i++) {
    cf[i] = (float)(cf[i] * sum);
    k[i] = round_even(cf[i] * 256.0f);
  }
}

void build_launch_plan(const Plan& P, const ResizeX* xt, const ResizeY* yt, const int2* rzb, LaunchPlan& LP) {
  const Geometry& G = P.G;
  LP = LaunchPlan{};
  for (int l = 1; l < G.nlevels; l++) {
    const LevelGeom &L = G.lv[l], &S = G.lv[l - 1];
    ResizeDesc& D = LP.rz[l];
    D.sw = S.w;
    D.sh = S.h;
    D.dw = L.w;
    D.dh = L.h;
    D.src_off = l == 1 ? -1 : S.off;
    D.dst_off = L.off;
    D.pyr_bytes = G.pyr_bytes;
    D.X = xt + L.xtab_off;
    D.Y = yt + L.ytab_off;
    D.bx = rzb + P.rzb_x[l];
    D.by = rzb + P.rzb_y[l];
    D.stride = G.rz_stride;
    D.rows = G.rz_rows;
    D.lc = G.rz_lc;
    D.strip = P.strip[l];
    if (P.strip[l]) {
      D.sbx = rzb + P.rsb_x[l];
      D.sby = rzb + P.rsb_y[l];
    }
  }
}

// Whether level l (tables already in P) can run k_resize_strip.  A lane covers a group of 4 output
// columns with one 8-byte window of a footprint row, a wave walks its strip's source rows once in
// order, and a tile's footprint has to fit the kernel's compile-time LDS shape:
//   - sx1(last) - sx0(first) <= 7 in every aligned group of 4 output columns;
//   - every output row reads rows sy0, sy0 + 1, and sy0 advances by 1 or 2 per output row;
//   - every 256-column tile spans <= kRsStride source bytes, every kRsTH-row tile <= kRsRows rows.
// Every level of a 1.2 pyramid passes; whatever does not keeps k_resize.
bool strip_resize_ok(const Plan& P, int l) {
#ifdef ORBX_RZ_GENERAL  // A/B and probe builds: every level on k_resize
  return false;
#endif
  const LevelGeom& L = P.G.lv[l];
  const ResizeX* X = P.xt.data() + L.xtab_off;
  const ResizeY* Y = P.yt.data() + L.ytab_off;
  for (int c = 0; c < L.w; c += 4)
    for (int k = c; k < std::min(c + 4, L.w); k++)
      if (X[k].sx0 < X[c].sx0 || X[k].sx1 < X[k].sx0 || X[k].sx1 - X[c].sx0 > 7) return false;
  for (int y = 0; y < L.h; y++) {
    if (Y[y].sy1 != Y[y].sy0 + 1) return false;
    if (y > 0 && (Y[y].sy0 - Y[y - 1].sy0 < 1 || Y[y].sy0 - Y[y - 1].sy0 > 2)) return false;
  }
  for (int ox = 0; ox < L.w; ox += kRsTW)
    if (X[std::min(ox + kRsTW, L.w) - 1].sx1 - X[ox].sx0 + 1 > kRsStride) return false;
  for (int oy = 0; oy < L.h; oy += kRsTH)
    if (Y[std::min(oy + kRsTH, L.h) - 1].sy1 - Y[oy].sy0 + 1 > kRsRows) return false;
  return true;
}

// Builds the per-geometry plan.  Level sizes: ComputePyramid
// (src/ORBextractor.cc:1219-1221); FAST cells: ComputeKeyPointsOctTree
// (:826-880); octree roots: DistributeOctTree (:567-570); resize tables:
// OpenCV 3.2 resizeGeneric_ coefficient setup.
orbx_status build_plan(const orbx_extractor_params& p, const Tables& t, int W, int H, Plan& P) {
  Geometry& G = P.G;
  std::memset(&G, 0, sizeof(G));
  G.nlevels = p.nlevels;
  G.width = W;
  G.height = H;
  G.ini_th = p.ini_th_fast;
  G.min_th = p.min_th_fast;
  long long pyr = 0, blur = 0;
  int cand = 0, oct = 0, ntiles = 0, node_cap = 64, cell_cap = 1;
  int lv_wmax[kMaxLevelsPlan] = {}, lv_hmax[kMaxLevelsPlan] = {};  // k_fast: largest cell per level
  P.cells.clear();
  P.tile_level.clear();
  P.xt.clear();
  P.yt.clear();
  P.rzb.clear();
  for (int l = 0; l < p.nlevels; l++) {
    LevelGeom& L = G.lv[l];
    L.w = round_even((float)W * t.inv_scale[l]);
    L.h = round_even((float)H * t.inv_scale[l]);
    if (L.w < 1 || L.h < 1 || L.w > 4095 || L.h > 4095) return ORBX_ERR_SIZE;
    L.off = l == 0 ? 0 : pyr;
    if (l > 0) pyr += (long long)L.w * L.h;
    // blurred level: tiles of 8 rows x 16 bytes (128 B), tile (ty, tx) at (ty * bstride/16 + tx) * 128,
    // row y of a tile at 16 * (y & 7): a 37x37 patch k_describe gathers covers 5-6 x 3-4 such
    // 128-B tiles (~20) against ~48 128-B lines in a row-major layout
    L.bstride = (L.w + 15) & ~15;
    L.boff = blur;
    blur += ((long long)L.bstride * ((L.h + 7) & ~7) + 255) & ~255LL;
    L.minBX = L.minBY = kEdgeThresholdHost - 3;
    L.maxBX = L.w - kEdgeThresholdHost + 3;
    L.maxBY = L.h - kEdgeThresholdHost + 3;
    L.scale = t.scale[l];
    L.kp_size = (float)(int)(31 * t.scale[l]);
    L.nfeat = t.nfeat[l];
    // FAST cells
    L.cell_begin = (int)P.cells.size();
    L.cand_begin = cand;
    const float width = (float)(L.maxBX - L.minBX), height = (float)(L.maxBY - L.minBY);
    const int nCols = (int)(width / 30), nRows = (int)(height / 30);
    if (width > 0 && height > 0 && nCols > 0 && nRows > 0) {
      const int wCell = (int)std::ceil(width / nCols), hCell = (int)std::ceil(height / nRows);
      for (int i = 0; i < nRows; i++) {
        const float iniY = (float)(L.minBY + i * hCell);
        float maxY = iniY + hCell + 6;
        if (iniY >= L.maxBY - 3) continue;
        if (maxY > L.maxBY) maxY = (float)L.maxBY;
        for (int j = 0; j < nCols; j++) {
          const float iniX = (float)(L.minBX + j * wCell);
          float maxX = iniX + wCell + 6;
          if (iniX >= L.maxBX - 6) continue;
          if (maxX > L.maxBX) maxX = (float)L.maxBX;
          CellInfo c{};
          c.level = (int16_t)l;
          c.x0 = (int16_t)((int)iniX + 3);
          c.y0 = (int16_t)((int)iniY + 3);
          c.x1 = (int16_t)((int)maxX - 4);
          c.y1 = (int16_t)((int)maxY - 4);
          if (c.x1 < c.x0 || c.y1 < c.y0) continue;
          const int cw = c.x1 - c.x0 + 1, ch = c.y1 - c.y0 + 1;
          if (cw > 60 || ch > 60) return ORBX_ERR_SIZE;  // k_fast LDS tile bound
          lv_wmax[l] = std::max(lv_wmax[l], cw);
          lv_hmax[l] = std::max(lv_hmax[l], ch);
          c.cap = ((cw + 1) / 2) * ((ch + 1) / 2);
          c.lw = L.w;
          c.loff = (int)L.off;
          // inline slots: a level-dependent share of the cap (cells cover more of the scene, and
          // keep more survivors, at the coarser levels: ~5 at level 0 to ~28 at level 7 on KITTI)
          c.kin = (int16_t)std::min(c.cap, 4 * (int)std::ceil(2.0 * std::pow(1.25, (double)l)));
          cand += c.cap;
          P.cells.push_back(c);
        }
      }
    }
    L.cell_end = (int)P.cells.size();
    L.cand_cap = cand - L.cand_begin;
    cell_cap = std::max(cell_cap, L.cell_end - L.cell_begin);
    // octree roots
    int nIni = 1;
    if (L.maxBY - L.minBY > 0) nIni = (int)std::round((float)(L.maxBX - L.minBX) / (L.maxBY - L.minBY));
    if (nIni < 1) nIni = 1;
    L.nIni = nIni;
    L.hX = (float)(L.maxBX - L.minBX) / nIni;
    L.oct_cap = std::max(L.nfeat + 3, 4 * nIni);
    L.oct_off = oct;
    oct += L.oct_cap;
    node_cap = std::max(node_cap, (L.oct_cap + 63) / 64 * 64);
    // blur tiles
    L.tiles_x = (L.w + kBlurTileW - 1) / kBlurTileW;
    L.tiles_y = (L.h + kBlurTileH - 1) / kBlurTileH;
    L.tile_begin = ntiles;
    ntiles += L.tiles_x * L.tiles_y;
    for (int q = 0; q < L.tiles_x * L.tiles_y; q++) P.tile_level.push_back(l);
    // resize tables (source = level l-1)
    if (l > 0) {
      const LevelGeom& S = G.lv[l - 1];
      const int sw = S.w, sh = S.h, dw = L.w, dh = L.h;
      const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
      L.xtab_off = (int)P.xt.size();
      for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)std::floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx + 1 >= sw && sx >= sw - 1) { fx = 0; sx = sw - 1; }
        ResizeX X;
        X.sx0 = sx;
        X.sx1 = std::min(sx + 1, sw - 1);
        X.a0 = (int16_t)round_even((1.f - fx) * 2048);
        X.a1 = (int16_t)round_even(fx * 2048);
        if (sx + 1 >= sw) {  // xmax region: D = S[sx]*2048
          X.a0 = 2048;
          X.a1 = 0;
        }
        P.xt.push_back(X);
      }
      L.ytab_off = (int)P.yt.size();
      for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)std::floor(fy);
        fy -= sy;
        ResizeY Y;
        Y.sy0 = std::min(std::max(sy, 0), sh - 1);
        Y.sy1 = std::min(std::max(sy + 1, 0), sh - 1);
        Y.b0 = (int16_t)round_even((1.f - fy) * 2048);
        Y.b1 = (int16_t)round_even(fy * 2048);
        P.yt.push_back(Y);
      }
    }
  }
  // k_fast LDS layout of a launch group, sized by its largest cell: window tile of H+6 rows at
  // stride S, score map (H+2) x S (one zero row/column each side), compass list W*H u16.  The
  // compass reads up to 6 rows past the tile for lanes below the region (masked): they land in the
  // map or list, or past the allocation (reads as 0).  One-wave blocks per CU are LDS-bound and
  // k_fast is latency-bound (+1 / +2 KB of LDS per block measured +8 / +15 % time), so the stride
  // is the smallest the kernel is built for (40 for 31-32 px cells), and the levels whose cells fit
  // 5 KB (32 blocks per CU) get their own launch when taller cells of the other levels would not
  // (KITTI: levels 0-3 at 5.0 KB, levels 4-7 with their 38-40-row cells at 6.0 KB).
  {
    auto layout = [&](int wmax, int hmax, Geometry::FastGroup& g) {
      g.s = wmax + 6 <= 40 ? 40 : wmax + 6 <= 48 ? 48 : 80;
      g.rp = wmax <= 32 ? 2 : 1;
      g.tile_bytes = ((hmax + 6) * g.s + 15) & ~15;
      g.map_bytes = ((hmax + 2) * g.s + 15) & ~15;
      g.smem = g.tile_bytes + g.map_bytes + 2 * wmax * hmax;
      // window loads per lane: a load covers 64 / (chunks per row) window rows (21 at S = 40 / 48, 12
      // at S = 80).  The tallest cell the grid above can make is 53 rows (a single cell row, whose
      // window is clipped to the region: 59 rows; two or more rows give hCell <= 45), so k_fast is
      // built for 2 or 3 loads at S = 40 / 48 and 4 or 5 at S = 80 (checked below)
      const int rpi = 64 / ((g.s + 15) / 16);
      g.nk = std::max(g.s == 80 ? 4 : 2, (hmax + 6 + rpi - 1) / rpi);
    };
    constexpr int kFastLdsFit = 5 * 1024;
    int split = 0, wa = 1, ha = 1;  // levels [0, split) fit kFastLdsFit together
    for (int l = 0; l < p.nlevels; l++) {
      Geometry::FastGroup g{};
      layout(std::max(wa, lv_wmax[l]), std::max(ha, lv_hmax[l]), g);
      if (g.smem > kFastLdsFit) break;
      wa = std::max(wa, lv_wmax[l]);
      ha = std::max(ha, lv_hmax[l]);
      split = l + 1;
    }
    if (split == 0) split = p.nlevels;  // one launch
    auto group = [&](int l0, int l1, Geometry::FastGroup& g) {  // the cells of levels [l0, l1)
      int w = 1, h = 1;
      for (int l = l0; l < l1; l++) {
        w = std::max(w, lv_wmax[l]);
        h = std::max(h, lv_hmax[l]);
      }
      layout(w, h, g);
      g.c0 = G.lv[l0].cell_begin;
      g.c1 = G.lv[l1 - 1].cell_end;
    };
    G.n_fg = 0;
    group(0, split, G.fg[G.n_fg++]);
    if (split < p.nlevels) group(split, p.nlevels, G.fg[G.n_fg++]);
    for (int g = 0; g < G.n_fg; g++)
      if (G.fg[g].nk > (G.fg[g].s == 80 ? 5 : 3)) return ORBX_ERR_SIZE;  // no k_fast instance stages that many
  }
  // k_resize staging bound: source footprint of every 128x16 output tile
  G.rz_rows = 1;
  G.rz_stride = 16;
  // (the same bounds go into rzb, where a block finds its footprint without walking the tables:
  // level l's tw x th tiles, its tile columns from x_at and its tile rows from y_at)
  auto push_bounds = [&](int l, int tw, int th, int& x_at, int& y_at) {
    const LevelGeom& L = G.lv[l];
    x_at = (int)P.rzb.size();
    for (int ox = 0; ox < L.w; ox += tw)
      P.rzb.push_back(make_int2(P.xt[L.xtab_off + ox].sx0, P.xt[L.xtab_off + std::min(ox + tw, L.w) - 1].sx1));
    y_at = (int)P.rzb.size();
    for (int oy = 0; oy < L.h; oy += th)
      P.rzb.push_back(make_int2(P.yt[L.ytab_off + oy].sy0, P.yt[L.ytab_off + std::min(oy + th, L.h) - 1].sy1));
  };
  for (int l = 1; l < G.nlevels; l++) {
    push_bounds(l, kRzTW, kRzTH, P.rzb_x[l], P.rzb_y[l]);
    for (int i = P.rzb_x[l]; i < P.rzb_y[l]; i++)
      G.rz_stride = std::max(G.rz_stride, (P.rzb[i].y - P.rzb[i].x + 1 + 15) / 16 * 16);
    for (int i = P.rzb_y[l]; i < (int)P.rzb.size(); i++) G.rz_rows = std::max(G.rz_rows, P.rzb[i].y - P.rzb[i].x + 1);
  }
  if (G.rz_rows > kRzMaxRows || (size_t)G.rz_rows * (G.rz_stride + 2 * kRzTW) > 64 * 1024) return ORBX_ERR_SIZE;
  // path choice per level; the strip tiles' bounds after k_resize's (which stay, whatever the path)
  P.rzb_n = (int)P.rzb.size();
  for (int l = 1; l < G.nlevels; l++) {
    P.strip[l] = strip_resize_ok(P, l);
    if (P.strip[l]) push_bounds(l, kRsTW, kRsTH, P.rsb_x[l], P.rsb_y[l]);
  }
  G.rz_lc = 0;
  while ((1 << G.rz_lc) < G.rz_stride / 16) G.rz_lc++;
  // every footprint row must be loaded: rows per thread = ceil(rz_rows / (256 >> rz_lc)) <= the kernel's 4
  if (G.rz_lc > 8 || (G.rz_rows + (256 >> G.rz_lc) - 1) / (256 >> G.rz_lc) > (kRzMaxRows + 15) / 16) return ORBX_ERR_SIZE;
  G.pyr_bytes = (pyr + 255) & ~255LL;
  G.blur_bytes = (blur + 255) & ~255LL;
  G.ncells = (int)P.cells.size();
  G.cand_total = std::max(cand, 1);
  {  // the cells' inline slots back to back, then their overflow slots (cand_total slots in all)
    int in_off = 0, ov_off = 0;
    for (const CellInfo& c : P.cells) in_off += c.kin;
    const int n_in = in_off;
    in_off = 0;
    for (CellInfo& c : P.cells) {
      c.cand_off = in_off;
      c.ovf_off = n_in + ov_off;
      in_off += c.kin;
      ov_off += c.cap - c.kin;
    }
  }
  G.oct_total = oct;
  G.max_kps = oct;
  G.ntiles = ntiles;
  if (node_cap > 8192) return ORBX_ERR_SIZE;
  if (octree_smem_bytes(node_cap, cell_cap, 0) > 160 * 1024 - 1024) return ORBX_ERR_SIZE;
  // k_octree launch groups: the levels with more than 0.4 x level 0's pixels as 512-thread blocks
  // whose candidate slots fill the block up to 50 KB with the kernel's static LDS (three blocks must
  // fit the CU's 160 KB -- the VGPR limit allows three; at 53 KB the allocation granularity left two
  // and the kernel ran 15 % slower; at least 1024 slots, never more than a level can hold), the
  // smaller ones as 256-thread blocks in <= 24 KB
  // (six per CU: their blocks are short and barrier-bound, so more of them in flight is what pays;
  // 0.231 -> 0.212 ms per step; 128-thread blocks, other budgets and splits measured no better,
  // profiles/r04/ab_octree_groups.txt)
  {
    const long long P0 = (long long)G.lv[0].w * G.lv[0].h;
    int split = 1;
    while (split < p.nlevels && (long long)G.lv[split].w * G.lv[split].h * 10 > 4 * P0) split++;
    auto group = [&](int l0, int l1, int nt, long long budget, OctGroup& g) {
      g.l0 = l0;
      g.l1 = l1;
      g.nt = nt;
      g.node_cap = 64;
      g.cell_cap = 1;
      int mc = 1;
      for (int l = l0; l < l1; l++) {
        g.node_cap = std::max(g.node_cap, (G.lv[l].oct_cap + 63) / 64 * 64);
        g.cell_cap = std::max(g.cell_cap, G.lv[l].cell_end - G.lv[l].cell_begin);
        mc = std::max(mc, G.lv[l].cand_cap);
      }
      const long long base = (long long)octree_smem_bytes(g.node_cap, g.cell_cap, 0);
      long long kc = (budget - 512 - base) / 6;
      kc = std::max(kc, 1024LL) & ~63LL;
      kc = std::min(kc, (long long)(mc + 63) / 64 * 64);
      while (kc > 64 && (long long)octree_smem_bytes(g.node_cap, g.cell_cap, (int)kc) > 160 * 1024 - 1024) kc -= 64;
      g.kcap = (int)kc;
      // the count pyramid's depth: the deepest whose LDS, for the group's largest root count, fits in
      // what the generic path takes anyway (the block's LDS, and the blocks per CU, stay as they were)
      g.nini = 1;
      g.span = 2;
      for (int l = l0; l < l1; l++) {
        g.nini = std::max(g.nini, G.lv[l].nIni);
        g.span = std::max(g.span, std::max(G.lv[l].maxBX - G.lv[l].minBX, 0) + std::max(G.lv[l].maxBY - G.lv[l].minBY, 0) + 2);
      }
      g.depth = 0;
      g.pcap = g.kcap;
      const long long have = (long long)octree_smem_bytes(g.node_cap, g.cell_cap, g.kcap);
      for (int d = kOctMaxDepth; d >= 1 && g.depth == 0; d--)
        if (g.nini < (1 << 10) && oct_pyr_layout(g.node_cap, g.cell_cap, g.kcap, g.span, g.nini, d).bytes <= have) g.depth = d;
      // what the chosen depth leaves of the group's LDS holds more candidates, up to a level's most
      if (g.depth > 0) {
        const long long left = have - oct_pyr_layout(g.node_cap, g.cell_cap, g.kcap, g.span, g.nini, g.depth).bytes;
        g.pcap = (int)std::min((long long)g.kcap + left / 4 / 64 * 64, std::max((long long)g.kcap, (long long)(mc + 63) / 64 * 64));
      }
    };
    G.n_og = 0;
    group(0, split, 512, 50 * 1024, G.og[G.n_og++]);
    if (split < p.nlevels) group(split, p.nlevels, 256, 24 * 1024, G.og[G.n_og++]);
    // one or two images (the host-API calls): every level in ONE launch of 512-thread blocks with
    // the CU's LDS to spend -- a handful of blocks, so the groups' two launches would only run one
    // after the other
    group(0, p.nlevels, 512, 150 * 1024, G.og_all);
    // ... on the generic path alone (depth 0).  This row's blocks each have a CU to themselves, where
    // the generic path's candidate passes cost little and the pyramid's fixed work (tables, clear,
    // sums) does not pay: the single stereo frame measured 0.252 ms (parent) against 0.265 (depth 5)
    // and 0.282 (depth 6), five and three alternating pairs, profiles/r13/ab_single_frame.txt
    G.og_all.depth = 0;
  }
  return ORBX_OK;
}

bool params_ok(const orbx_extractor_params* p) {
  return p && p->nlevels >= 1 && p->nlevels <= kMaxLevelsPlan && p->scale_factor > 0.f && p->nfeatures >= 0;
}

}  // namespace orbx

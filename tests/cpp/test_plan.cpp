// test_plan.cpp -- the extraction plan (csrc/plan.hip) and the block-layout cursor (csrc/orbx_extractor.h)
// on the host alone: no HIP call is made, so it runs without a device (tests/test_plan.py builds it with
// the address and undefined-behaviour sanitizers and bounds-checked containers, and runs it as a child
// process).  For every plan it builds it asserts what the kernels of extract.hip rely on unguarded.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../orb_slam2_commit_amd/csrc/orbx_extractor.h"

using namespace orbx;

static int g_checks = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    g_checks++;                                                   \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static int cdiv(int a, int b) { return (a + b - 1) / b; }

static orbx_extractor_params params(int nfeatures, float sf = 1.2f, int nlevels = 8) {
  orbx_extractor_params p{};
  p.nfeatures = nfeatures;
  p.scale_factor = sf;
  p.nlevels = nlevels;
  p.ini_th_fast = 20;
  p.min_th_fast = 7;
  return p;
}

static orbx_status build(const orbx_extractor_params& p, int W, int H, Plan& P) {
  CHECK(params_ok(&p));
  return build_plan(p, make_tables(p), W, H, P);
}

struct Range {
  long long b, e;
};
// pairwise disjoint, all inside [0, limit)
static void check_disjoint_within(std::vector<Range> v, long long limit) {
  std::sort(v.begin(), v.end(), [](const Range& a, const Range& b) { return a.b < b.b; });
  long long end = 0;
  for (const Range& r : v) {
    CHECK(r.b >= end && r.e >= r.b);
    end = r.e;
  }
  CHECK(end <= limit);
}

static void check_levels(const Plan& P) {
  const Geometry& G = P.G;
  std::vector<Range> pyr, blur;
  int ntiles = 0;
  for (int l = 0; l < G.nlevels; l++) {
    const LevelGeom& L = G.lv[l];
    CHECK(L.w >= 1 && L.h >= 1 && L.w <= 4095 && L.h <= 4095);
    if (l >= 1) pyr.push_back({L.off, L.off + (long long)L.w * L.h});
    CHECK(L.bstride % 16 == 0 && L.bstride >= L.w && L.boff % 256 == 0);
    blur.push_back({L.boff, L.boff + (long long)L.bstride * ((L.h + 7) / 8 * 8)});
    CHECK(L.tile_begin == ntiles && L.tiles_x == cdiv(L.w, kBlurTileW) && L.tiles_y == cdiv(L.h, kBlurTileH));
    for (int q = 0; q < L.tiles_x * L.tiles_y; q++) CHECK(P.tile_level[ntiles + q] == l);
    ntiles += L.tiles_x * L.tiles_y;
  }
  CHECK(G.ntiles == ntiles && (int)P.tile_level.size() == ntiles);
  check_disjoint_within(pyr, G.pyr_bytes);
  check_disjoint_within(blur, G.blur_bytes);
}

// every candidate slot of the image's block belongs to exactly one cell (inline or overflow)
static void check_cells(const Plan& P) {
  const Geometry& G = P.G;
  CHECK(G.ncells == (int)P.cells.size());
  if (P.cells.empty()) {
    CHECK(G.cand_total == 1);
    return;
  }
  std::vector<int> owner((size_t)G.cand_total, 0);
  for (int l = 0, c = 0; l < G.nlevels; l++) {
    const LevelGeom& L = G.lv[l];
    CHECK(L.cell_begin == c && L.cell_end >= c);
    int cap = 0;
    for (; c < L.cell_end; c++) {
      const CellInfo& I = P.cells[c];
      CHECK(I.level == l && I.lw == L.w && (l == 0 || I.loff == L.off));
      // the window k_fast loads (3 px around the region) lies inside the level
      CHECK(I.x0 >= 3 && I.y0 >= 3 && I.x1 >= I.x0 && I.y1 >= I.y0 && I.x1 + 3 < L.w && I.y1 + 3 < L.h);
      CHECK(I.kin >= 0 && I.kin <= I.cap && I.cand_off >= 0 && I.ovf_off >= 0);
      CHECK((long long)I.cand_off + I.kin <= G.cand_total && (long long)I.ovf_off + I.cap - I.kin <= G.cand_total);
      for (int q = 0; q < I.cap; q++) owner[cell_slot(I, q)]++;
      cap += I.cap;
    }
    CHECK(L.cand_cap == cap);
  }
  for (int v : owner) CHECK(v == 1);
}

static void check_fast_groups(const Plan& P) {
  const Geometry& G = P.G;
  CHECK(G.n_fg >= 1 && G.n_fg <= 2 && G.fg[0].c0 == 0 && G.fg[G.n_fg - 1].c1 == G.ncells);
  for (int g = 0; g < G.n_fg; g++) {
    const Geometry::FastGroup& F = G.fg[g];
    if (g > 0) CHECK(F.c0 == G.fg[g - 1].c1);  // consecutive ranges: every cell in exactly one group
    CHECK(F.c1 >= F.c0);
    CHECK(F.s == 40 || F.s == 48 || F.s == 80);
    CHECK(F.nk >= (F.s == 80 ? 4 : 2) && F.nk <= (F.s == 80 ? 5 : 3));  // the k_fast instances built
    const int rpi = 64 / ((F.s + 15) / 16);  // window rows one load per lane covers
    int wmax = 1, hmax = 1;
    for (int c = F.c0; c < F.c1; c++) {
      const int w = P.cells[c].x1 - P.cells[c].x0 + 1, h = P.cells[c].y1 - P.cells[c].y0 + 1;
      CHECK(w + 6 <= F.s);
      CHECK(h + 6 <= F.nk * rpi);
      CHECK((w <= 32) || F.rp == 1);
      wmax = std::max(wmax, w);
      hmax = std::max(hmax, h);
    }
    CHECK(F.tile_bytes == (((hmax + 6) * F.s + 15) & ~15) && F.map_bytes == (((hmax + 2) * F.s + 15) & ~15));
    CHECK(F.smem == F.tile_bytes + F.map_bytes + 2 * wmax * hmax);
    CHECK(F.smem <= 64 * 1024);
  }
}

static void check_octree_groups(const Plan& P) {
  const Geometry& G = P.G;
  auto check_group = [&](const OctGroup& g) {
    CHECK(g.l0 >= 0 && g.l1 > g.l0 && g.l1 <= G.nlevels && (g.nt == 512 || g.nt == 256));
    CHECK(g.kcap >= 64 && g.kcap % 64 == 0 && g.node_cap % 64 == 0 && g.node_cap <= 8192);
    CHECK(octree_smem_bytes(g.node_cap, g.cell_cap, g.kcap) <= 160 * 1024 - 1024);
    for (int l = g.l0; l < g.l1; l++) {
      CHECK(g.node_cap >= G.lv[l].oct_cap);
      CHECK(g.cell_cap >= G.lv[l].cell_end - G.lv[l].cell_begin);
    }
  };
  CHECK(G.n_og >= 1 && G.n_og <= 2 && G.og[0].l0 == 0 && G.og[G.n_og - 1].l1 == G.nlevels);
  for (int g = 0; g < G.n_og; g++) {
    if (g > 0) CHECK(G.og[g].l0 == G.og[g - 1].l1);
    check_group(G.og[g]);
  }
  CHECK(G.og_all.l0 == 0 && G.og_all.l1 == G.nlevels);
  check_group(G.og_all);
  int oct = 0;
  for (int l = 0; l < G.nlevels; l++) {
    CHECK(G.lv[l].oct_off == oct && G.lv[l].oct_cap >= std::max(G.lv[l].nfeat, 4 * G.lv[l].nIni) && G.lv[l].nIni >= 1);
    oct += G.lv[l].oct_cap;
  }
  CHECK(G.oct_total == oct && G.max_kps == oct);
}

// strip_resize_ok's four conditions, recomputed from the level's tables
static bool strip_conditions(const ResizeX* X, const ResizeY* Y, int dw, int dh) {
  for (int c = 0; c < dw; c += 4) {  // a lane's 4 columns read one 8-byte window starting at its first tap
    int lo = X[c].sx0, hi = X[c].sx1;
    for (int k = c; k < std::min(c + 4, dw); k++) {
      lo = std::min(lo, X[k].sx0);
      hi = std::max(hi, std::max(X[k].sx0, X[k].sx1));
    }
    if (lo != X[c].sx0 || hi - lo > 7) return false;
  }
  for (int y = 0; y < dh; y++) {  // rows sy0, sy0 + 1; sy0 advances by 1 or 2
    if (Y[y].sy1 - Y[y].sy0 != 1) return false;
    if (y > 0 && Y[y].sy0 - Y[y - 1].sy0 != 1 && Y[y].sy0 - Y[y - 1].sy0 != 2) return false;
  }
  for (int t = 0; t < cdiv(dw, kRsTW); t++)  // a tile's footprint fits the kernel's LDS shape
    if (X[std::min((t + 1) * kRsTW, dw) - 1].sx1 - X[t * kRsTW].sx0 + 1 > kRsStride) return false;
  for (int t = 0; t < cdiv(dh, kRsTH); t++)
    if (Y[std::min((t + 1) * kRsTH, dh) - 1].sy1 - Y[t * kRsTH].sy0 + 1 > kRsRows) return false;
  return true;
}

static void check_resize(const Plan& P) {
  const Geometry& G = P.G;
  LaunchPlan LP;
  build_launch_plan(P, P.xt.data(), P.yt.data(), P.rzb.data(), LP);
  const ResizeX* xe = P.xt.data() + P.xt.size();
  const ResizeY* ye = P.yt.data() + P.yt.size();
  const int2 *rb = P.rzb.data(), *re = rb + P.rzb.size();
  CHECK(P.rzb_n >= 0 && P.rzb_n <= (int)P.rzb.size());
  for (int l = 1; l < G.nlevels; l++) {
    const ResizeDesc& D = LP.rz[l];
    CHECK(D.sw == G.lv[l - 1].w && D.sh == G.lv[l - 1].h && D.dw == G.lv[l].w && D.dh == G.lv[l].h);
    CHECK(D.dst_off == G.lv[l].off && D.src_off == (l == 1 ? -1 : G.lv[l - 1].off) && D.pyr_bytes == G.pyr_bytes);
    // every table pointer inside its table with the level's full run behind it
    CHECK(D.X >= P.xt.data() && D.X + D.dw <= xe);
    CHECK(D.Y >= P.yt.data() && D.Y + D.dh <= ye);
    const int ntx = cdiv(D.dw, kRzTW), nty = cdiv(D.dh, kRzTH);
    CHECK(D.bx >= rb && D.bx + ntx <= rb + P.rzb_n && D.by >= rb && D.by + nty <= rb + P.rzb_n);
    for (int i = 0; i < D.dw; i++) CHECK(D.X[i].sx0 >= 0 && D.X[i].sx0 <= D.X[i].sx1 && D.X[i].sx1 < D.sw);
    for (int i = 0; i < D.dh; i++) CHECK(D.Y[i].sy0 >= 0 && D.Y[i].sy0 <= D.Y[i].sy1 && D.Y[i].sy1 < D.sh);
    for (int t = 0; t < ntx; t++) {  // k_resize stages [bx.x, bx.y] at the plan's stride
      CHECK(D.bx[t].x == D.X[t * kRzTW].sx0 && D.bx[t].y == D.X[std::min((t + 1) * kRzTW, D.dw) - 1].sx1);
      CHECK(D.bx[t].y - D.bx[t].x + 1 <= D.stride);
    }
    for (int t = 0; t < nty; t++) {
      CHECK(D.by[t].x == D.Y[t * kRzTH].sy0 && D.by[t].y == D.Y[std::min((t + 1) * kRzTH, D.dh) - 1].sy1);
      CHECK(D.by[t].y - D.by[t].x + 1 <= D.rows);
    }
    CHECK(D.stride == G.rz_stride && D.rows == G.rz_rows && D.lc == G.rz_lc && D.stride % 16 == 0);
    CHECK(D.rows <= kRzMaxRows && (16 << D.lc) >= D.stride && D.lc <= 8);
    CHECK((size_t)D.rows * (D.stride + 2 * kRzTW) <= 64 * 1024);
    CHECK((D.strip != 0) == P.strip[l]);
    if (D.strip) {
      const int stx = cdiv(D.dw, kRsTW), sty = cdiv(D.dh, kRsTH);
      CHECK(D.sbx >= rb + P.rzb_n && D.sbx + stx <= re && D.sby >= rb + P.rzb_n && D.sby + sty <= re);
      for (int t = 0; t < stx; t++)
        CHECK(D.sbx[t].x == D.X[t * kRsTW].sx0 && D.sbx[t].y == D.X[std::min((t + 1) * kRsTW, D.dw) - 1].sx1);
      for (int t = 0; t < sty; t++)
        CHECK(D.sby[t].x == D.Y[t * kRsTH].sy0 && D.sby[t].y == D.Y[std::min((t + 1) * kRsTH, D.dh) - 1].sy1);
      CHECK(strip_conditions(D.X, D.Y, D.dw, D.dh));
    }
  }
}

static void check_plan(const orbx_extractor_params& p, int W, int H, Plan& P) {
  CHECK(build(p, W, H, P) == ORBX_OK);
  CHECK(P.G.nlevels == p.nlevels && P.G.width == W && P.G.height == H);
  check_levels(P);
  check_cells(P);
  check_fast_groups(P);
  check_octree_groups(P);
  check_resize(P);
}

static int cells_of(const Plan& P, int l) { return P.G.lv[l].cell_end - P.G.lv[l].cell_begin; }

static void test_geometries() {
  Plan P;
  check_plan(params(2000), 1241, 376, P);
#ifndef ORBX_RZ_GENERAL
  for (int l = 1; l < 8; l++) CHECK(P.strip[l]);  // every level of a 1.2 pyramid takes the strip path
#endif
  CHECK(P.G.n_fg == 2 && P.G.n_og == 2);
  check_plan(params(1200), 752, 480, P);
  check_plan(params(1000), 640, 480, P);
  check_plan(params(300), 253, 199, P);  // the odd size of tests/test_launch_descriptors.py
  check_plan(params(1000, 1.2f, 1), 640, 480, P);  // one level: no resize tables at all
  CHECK(P.xt.empty() && P.yt.empty() && P.rzb.empty() && P.G.n_og == 1);
  // no cells anywhere: level 0's border box is 32 x 16, under one 30-px cell row
  check_plan(params(500), 64, 48, P);
  CHECK(P.cells.empty() && P.G.cand_total == 1);
  // cells at the lower levels, none at the top ones (level 7 is 33 x 28: an empty border box)
  check_plan(params(500), 120, 100, P);
  CHECK(cells_of(P, 0) > 0 && cells_of(P, 7) == 0 && P.G.lv[7].maxBY <= P.G.lv[7].minBY);
  // level 0 a single row of cells at its tallest: a border box 59 rows high gives a 53-row region
  check_plan(params(500), 640, 91, P);
  CHECK(cells_of(P, 0) == 20 && P.cells[0].y1 - P.cells[0].y0 + 1 == 53);
  check_plan(params(0), 640, 480, P);  // nfeatures 0: every quota 0, the octree lists still hold their roots
  for (int l = 0; l < 8; l++) CHECK(P.G.lv[l].nfeat == 0 && P.G.lv[l].oct_cap >= 4 * P.G.lv[l].nIni);
  // other pyramids: 2.0 (no level passes the strip conditions: k_resize everywhere), 16 levels of 1.1
  check_plan(params(1000, 2.0f, 4), 640, 480, P);
  for (int l = 1; l < 4; l++) CHECK(!P.strip[l]);
  check_plan(params(1000, 1.1f, 16), 640, 480, P);
  check_plan(params(5000), 4095, 4095, P);  // the largest level the plan takes
}

static void test_refusals() {
  Plan P;
  // level 0 is 5000 wide: the level-size check (w > 4095) of the level loop
  CHECK(build(params(500), 5000, 240, P) == ORBX_ERR_SIZE);
  // 16 levels on 7 rows: level 15 is cvRound(7 / 1.2^15 = 0.454) = 0 rows, the same check (h < 1)
  CHECK(build(params(500, 1.2f, 16), 640, 7, P) == ORBX_ERR_SIZE);
  CHECK(build(params(500, 1.2f, 15), 640, 7, P) == ORBX_OK);
  // a 4.0 pyramid: a 32-row output tile reads ~128 source rows, the k_resize staging check (rz_rows > 64)
  CHECK(build(params(500, 4.0f, 3), 640, 480, P) == ORBX_ERR_SIZE);
  // The cell-size check (a cell over 60 x 60) has no geometry that fires it: a box of `width` pixels is cut
  // into (int)(width / 30) columns, so one column leaves a clipped cell of width - 6 <= 53 and two or more
  // give ceil(width / n) <= 45 (rows alike).  Every level size a plan can hold, on both axes:
  for (int s = 1; s <= 4095; s++) {
    const float width = (float)(s - 2 * (kEdgeThresholdHost - 3));
    const int n = (int)(width / 30);
    if (n < 1) continue;
    const int cell = (int)std::ceil(width / n);
    CHECK((n == 1 ? (int)width - 6 : cell) <= 53);
  }
  for (int s = 33; s < 700; s += 13) {  // and as built
    CHECK(build(params(500), s, 700 - s + 33, P) == ORBX_OK);
    for (const CellInfo& c : P.cells) CHECK(c.x1 - c.x0 + 1 <= 53 && c.y1 - c.y0 + 1 <= 53);
  }
  orbx_extractor_params bad = params(500, 1.2f, kMaxLevelsPlan + 1);
  CHECK(!params_ok(&bad) && !params_ok(nullptr));
}

// the host paths' device blocks: fields in take() order behind the 256-byte header, aligned, disjoint
struct Field {
  size_t off, bytes;
};
static void check_block(const std::vector<Field>& f, size_t end) {
  size_t at = 256;
  for (const Field& x : f) {
    CHECK(x.off % 256 == 0 && x.off >= at);
    at = x.off + x.bytes;
  }
  CHECK(end >= at && end % 256 == 0 && end - at < 256);
}
template <class T>
static Field take(BlockCursor& c, size_t count) {
  return {c.take<T>(count), count * sizeof(T)};
}

static void test_cursor() {
  static_assert(sizeof(orbx_keypoint) == 28, "keypoint record");
  CHECK(BlockCursor().end() == 256);
  for (size_t kc : {(size_t)1, (size_t)1203, (size_t)2257, (size_t)4096}) {
    {  // orbx_extract (orbx_stereo_match reads this block in place)
      BlockCursor c;
      const std::vector<Field> f = {take<orbx_keypoint>(c, kc), take<uint8_t>(c, kc * 32)};
      check_block(f, c.end());
      CHECK(f[0].off == 256);
    }
    {  // orbx_frame_stereo: keypoints and descriptors of two images, uRight, depth
      BlockCursor c;
      const std::vector<Field> f = {take<orbx_keypoint>(c, 2 * kc), take<uint8_t>(c, 2 * kc * 32), take<float>(c, kc),
                                    take<float>(c, kc)};
      check_block(f, c.end());
    }
    {  // orbx_frame_rgbd: keypoints, undistorted keypoints, descriptors, uRight, depth
      BlockCursor c;
      const std::vector<Field> f = {take<orbx_keypoint>(c, kc), take<orbx_keypoint>(c, kc), take<uint8_t>(c, kc * 32),
                                    take<float>(c, kc), take<float>(c, kc)};
      check_block(f, c.end());
    }
    for (size_t nR : {(size_t)0, (size_t)7, kc}) {  // orbx_debug_stereo_keypoints: nL = kc left, nR right keypoints
      BlockCursor c;
      const std::vector<Field> f = {take<orbx_keypoint>(c, kc), take<orbx_keypoint>(c, nR), take<uint8_t>(c, kc * 32),
                                    take<uint8_t>(c, nR * 32), take<float>(c, 2 * kc)};
      check_block(f, c.end());
    }
  }
  // the two stereo input shapes
  const orbx_keypoint* k = nullptr;
  const StereoSides two = StereoSides::handles(k, nullptr, nullptr, k, nullptr, nullptr);
  CHECK(two.L.k_stride == 0 && two.L.n_stride == 0 && two.L.step == 0 && two.L.off == 0);
  CHECK(two.R.k_stride == 0 && two.R.n_stride == 0 && two.R.step == 0 && two.R.off == 0);
  std::vector<orbx_keypoint> kps(4 * 5);
  std::vector<uint8_t> desc(4 * 5 * 32);
  std::vector<int32_t> cnt(4);
  const StereoSides il = StereoSides::interleaved(kps.data(), desc.data(), cnt.data(), 5);
  for (int f = 0; f < 2; f++) {  // frame f: images 2f (left) and 2f + 1 (right) of the batch
    CHECK(il.L.kps + f * il.L.k_stride == kps.data() + (2 * f) * 5 && il.R.kps + f * il.R.k_stride == kps.data() + (2 * f + 1) * 5);
    CHECK(il.L.desc + f * il.L.k_stride * 32 == desc.data() + (2 * f) * 5 * 32);
    CHECK(il.R.desc + f * il.R.k_stride * 32 == desc.data() + (2 * f + 1) * 5 * 32);
    CHECK(il.L.counts + f * il.L.n_stride == cnt.data() + 2 * f && il.R.counts + f * il.R.n_stride == cnt.data() + 2 * f + 1);
    CHECK(il.L.step * f + il.L.off == 2 * f && il.R.step * f + il.R.off == 2 * f + 1);
  }
}

int main() {
  test_geometries();
  test_refusals();
  test_cursor();
  std::printf("plan ok (%d checks)\n", g_checks);
  return 0;
}

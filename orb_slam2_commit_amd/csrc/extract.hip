// extract.hip -- ORB extraction (ORBextractor::operator(), src/ORBextractor.cc:1138-1211)
// as a batched chain of gfx950 kernels.  One launch per stage covers every
// image of the batch:
//
//   k_resize   x(nlevels-1)  ComputePyramid            src/ORBextractor.cc:1215-1250
//                            (k_resize_strip per level where the plan allows it, k_resize elsewhere)
//   k_fast                   per-cell FAST + fallback  src/ORBextractor.cc:843-915
//   k_octree                 DistributeOctTree         src/ORBextractor.cc:562-815
//   k_describe               IC_Angle + rBRIEF on the blurred level + scale
//                                                      src/ORBextractor.cc:77-152,1186-1207
//   k_blur                   whole-level GaussianBlur 7x7 s=2 into 8 x 16-B tiles (k_describe samples them)
//
// Integer/byte work throughout (HBM-bound); the only float math is the
// orientation/rotation and it is compiled without FP contraction so it rounds
// exactly like the CPU path.
#include <hip/hip_runtime.h>

#include <utility>

#include "orbx_device.h"
#include "orbx_internal.h"
#include "orbx_prof.h"

namespace orbx {

__constant__ float c_pattern_f[1024] = {  // bit_pattern_31_ as floats (exact small integers)
#include "brief_pattern_31.inc"
};
// IC_Angle's circle (umax, src/ORBextractor.cc:77-105) as per-lane byte masks over the 31x31
// box: lane = (row r = lane >> 1, half h = lane & 1) keeps byte b (column 16h + b) iff that
// column is inside row r - 15's span; lanes 62, 63 keep nothing
__constant__ uint4 c_icmask[64];
// sincos_det constants (orbx_device.h); external linkage keeps them loads, not folded immediates
__constant__ double c_sincos[23] = {
    6.36619772367581382433e-01,  // 2/pi
    1.57079632673412561417e+00,  // pi/2 hi
    6.07710050650619224932e-11,  // pi/2 lo
    1.0 / 51090942171709440000.0, -1.0 / 121645100408832000.0, 1.0 / 355687428096000.0,
    -1.0 / 1307674368000.0,       1.0 / 6227020800.0,           -1.0 / 39916800.0,
    1.0 / 362880.0,               -1.0 / 5040.0,                1.0 / 120.0,
    -1.0 / 6.0,  // sin: x^19 .. x^3
    1.0 / 2432902008176640000.0,  -1.0 / 6402373705728000.0,    1.0 / 20922789888000.0,
    -1.0 / 87178291200.0,         1.0 / 479001600.0,            -1.0 / 3628800.0,
    1.0 / 40320.0,                -1.0 / 720.0,                 1.0 / 24.0,
    -0.5};  // cos: x^20 .. x^2


constexpr int BS = 256;

typedef float float2v __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------- block scan
// Exclusive scan of a[0..n) in LDS (in place); returns the total. All NT threads call.
// Two barriers: after the wave totals are published every thread adds up the
// NT/64 totals below its own wave itself (no serial pass + second barrier);
// the trailing barrier orders the in-place writes before any other reader.
template <int NT, class T>
__device__ T block_scan_excl(T* a, int n) {
  __shared__ T wsum[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int chunk = (n + NT - 1) / NT;
  const int b = tid * chunk, e = min(n, b + chunk);
  T local = 0;
  for (int i = b; i < e; i++) local += a[i];
  T incl = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wsum[wid] = incl;
  __syncthreads();
  T before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; w++) {
    const T t = wsum[w];
    before += w < wid ? t : 0;
    total += t;
  }
  T run = before + incl - local;
  for (int i = b; i < e; i++) {
    const T v = a[i];
    a[i] = run;
    run += v;
  }
  __syncthreads();
  return total;
}

template <int NT>
__device__ int block_exclusive_scan(int* a, int n) {
  return block_scan_excl<NT, int>(a, n);
}

template <int NT>
__device__ int block_sum(int v) {
  __shared__ int red[NT / 64];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < NT / 64; w++) s += red[w];
  __syncthreads();
  return s;
}

// ------------------------------------------------------------ LDS staging
// Copy an nrows x ncols byte window (row stride `stride`, any alignment) into
// LDS (row stride ls).  Every load is an aligned dword and all MAXK loads of a
// thread are issued before the first LDS write, so the window costs one
// memory latency instead of one per row.  Needs ncols+6 <= 4*dwpr and the
// dword-rounded span to stay inside the buffer (true for level windows that
// start >= 3 bytes into a row and end >= 3 bytes before its end).
template <int MAXK>
__device__ __forceinline__ void window_to_lds(const uint8_t* base, size_t stride, int nrows, int ncols, uint8_t* lds,
                                              int ls, int tid, int nth) {
  const int dwpr = (ncols + 6) / 4 + 1;
  const int total = nrows * dwpr;
  uint32_t v[MAXK];
  int rr[MAXK], cc[MAXK];
#pragma unroll
  for (int k = 0; k < MAXK; k++) {
    const int q = tid + k * nth;
    v[k] = 0;
    rr[k] = -1;
    cc[k] = 0;
    if (q < total) {
      const int r = q / dwpr, j = q - r * dwpr;
      const uintptr_t a = (uintptr_t)(base + (size_t)r * stride);
      const int sh = (int)(a & 3);
      if (4 * j < sh + ncols) {
        v[k] = *((const uint32_t*)(a & ~(uintptr_t)3) + j);
        rr[k] = r;
        cc[k] = 4 * j - sh;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < MAXK; k++) {
    if (rr[k] < 0) continue;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int c = cc[k] + b;
      if (c >= 0 && c < ncols) lds[rr[k] * ls + c] = (uint8_t)(v[k] >> (8 * b));
    }
  }
}

// ------------------------------------------------------------------ resize
// cv::resize INTER_LINEAR 8U (OpenCV 3.2 fixed point, coefficient tables built
// on the host exactly as resizeGeneric_ does).  One block per 128x16 output
// tile, in three LDS phases:
//   1. the tile's source footprint (rows sy0(first)..sy1(last), cols
//      sx0(first)..sx1(last)) arrives as 16-B buffer loads at the unaligned row
//      positions, stored to 16-B aligned LDS rows (byte loads only for a chunk
//      straddling the level's last byte);
//   2. the horizontal pass once per footprint row and output column:
//      (S[sx0]*a0 + S[sx1]*a1) >> 4 as int16 (shared by the <= 2 output rows that
//      read each source row);
//   3. the vertical pass for 4 output columns per item:
//      ((b0*h0)>>16 + (b1*h1)>>16 + 2) >> 2 with v_mul_hi_u32_u24(b<<8, h<<8), packed
//      into one dword store.
//
// Everything block-uniform comes in the by-value ResizeDesc; the only scalar loads ahead of the
// footprint loads are the tile's two bound pairs (D.bx, D.by), issued together.
// Phase probe (build with -DORBX_RZ_PROBE only; tools/rz_probe.py): s_memtime ticks of a block's
// first wave in both resize kernels -- footprint to LDS (to the barrier), the horizontal pass
// (k_resize only, to its second barrier), the arithmetic up to the last store's issue, and the
// stores' drain -- then the level and the kernel (1: k_resize_strip).  One lane per block writes
// its 8 words with plain vector stores to a host-provided buffer, indexed by the level's first
// slot (ResizeDesc::probe_base) plus the block's logical index.
#ifdef ORBX_RZ_PROBE
__device__ unsigned int* rz_probe_buf;
__device__ unsigned int rz_probe_cap;  // blocks the buffer holds
#define RZ_TS(k) const unsigned long long ts##k = __builtin_amdgcn_s_memtime()
#define RZ_PROBE_WRITE(a, b, c, d, path)                                                                    \
  do {                                                                                                      \
    const unsigned slot = (unsigned)D.probe_base + ((unsigned)bi.z * D.rm.gy + (unsigned)bi.y) * D.rm.gx + (unsigned)bi.x; \
    if (threadIdx.x == 0 && rz_probe_buf && slot < rz_probe_cap) {                                          \
      unsigned int* o_ = rz_probe_buf + (size_t)slot * 8;                                                   \
      o_[0] = (unsigned int)(a), o_[1] = (unsigned int)(b), o_[2] = (unsigned int)(c), o_[3] = (unsigned int)(d); \
      o_[4] = (unsigned int)D.level, o_[5] = (path), o_[6] = 1, o_[7] = 0;                                  \
    }                                                                                                       \
  } while (0)
#else
#define RZ_TS(k)
#define RZ_PROBE_WRITE(a, b, c, d, path)
#endif

__global__ __launch_bounds__(BS) void k_resize(ResizeDesc D, const uint8_t* __restrict__ in, size_t in_pitch,
                                               uint8_t* __restrict__ pyr) {
  extern __shared__ __align__(16) uint8_t rz_smem[];
  RZ_TS(0);
  const int3 bi = xcd_block3(D.rm);
  const int img = bi.z, tid = threadIdx.x;
  const int2 fx = D.bx[bi.x], fy = D.by[bi.y];
  const int ox0 = bi.x * kRzTW, oy0 = bi.y * kRzTH;
  const int nx = min(kRzTW, D.dw - ox0), ny = min(kRzTH, D.dh - oy0);
  const ResizeX* X = D.X + ox0;
  const ResizeY* Y = D.Y + oy0;
  const int cx0 = fx.x, span = fx.y - cx0 + 1;
  const int ry0 = fy.x, nrows = fy.y - ry0 + 1;
  const int stride = D.stride;
  uint8_t* tin = rz_smem;
  int16_t* hb = (int16_t*)(rz_smem + D.rows * stride);  // [rows][kRzTW]
  // (both candidates computed, then selected: as a branch each arm would fetch its kernel arguments
  // itself, one more serial wait)
  const uint8_t* const src0 = in + (size_t)img * in_pitch;
  const uint8_t* const srcl = pyr + (size_t)img * D.pyr_bytes + D.src_off;
  const uint8_t* src = D.src_off < 0 ? src0 : srcl;
  const int swh = D.sw * D.sh;
  // the coefficient entries this thread needs later load first, beside the footprint: every
  // global load of the block is then in flight before the first wait (they used to trail the
  // barriers, one round trip each)
  const int hc = tid & (kRzTW - 1);
  const ResizeX xc = X[hc < nx ? hc : 0];
  constexpr int kVIt = kRzTH * (kRzTW / 4) / BS;  // vertical items per thread
  ResizeY yv[kVIt];
#pragma unroll
  for (int k = 0; k < kVIt; k++) {
    const int i = (tid + k * BS) / (kRzTW / 4);
    yv[k] = Y[i < ny ? i : 0];
  }
  // 1. footprint -> LDS: lane = (row, 16-B chunk) with a power-of-two lane count per row (the
  //    widest span's chunks; no division), all of a thread's chunk loads issued before their stores
  {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, (short)0, swh, 0x00020000);
    const int nch = (span + 15) >> 4;
    const int lc = D.lc;  // log2(chunk lanes per row)
    const int c = tid & ((1 << lc) - 1), r0 = tid >> lc, rstep = BS >> lc;
    constexpr int kRzLd = (kRzMaxRows + 15) / 16;  // >= rows per thread when >= 16 rows per step
    uint4 v[kRzLd];
#pragma unroll
    for (int u = 0; u < kRzLd; u++) {
      const int r = r0 + u * rstep;
      const int o = (ry0 + r) * D.sw + cx0 + 16 * c;
      v[u] = make_uint4(0, 0, 0, 0);
      if (r < nrows && c < nch) {
        if (o + 16 <= swh) {
          const auto t = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0);
          v[u] = make_uint4(t[0], t[1], t[2], t[3]);
        } else {  // last bytes of the level: byte loads, each range-checked (outside -> 0, never used)
          uint32_t w4[4] = {0, 0, 0, 0};
#pragma unroll
          for (int b = 0; b < 16; b++)
            w4[b >> 2] |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, o + b, 0, 0) << (8 * (b & 3));
          v[u] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kRzLd; u++) {
      const int r = r0 + u * rstep;
      if (r < nrows && c < nch) *(uint4*)&tin[r * stride + 16 * c] = v[u];
    }
  }
  __syncthreads();
  RZ_TS(1);
  // 2. horizontal pass: thread = one output column, rows strided by BS / kRzTW
  if (hc < nx) {
    const int s0 = xc.sx0 - cx0, s1 = xc.sx1 - cx0, a0 = xc.a0, a1 = xc.a1;
    // (the first row is wave-uniform: a scalar loop, no exec-mask bookkeeping per row)
    for (int r = __builtin_amdgcn_readfirstlane(tid / kRzTW); r < nrows; r += BS / kRzTW) {
      const uint8_t* t = tin + r * stride;
      hb[r * kRzTW + hc] = (int16_t)((t[s0] * a0 + t[s1] * a1) >> 4);
    }
  }
  __syncthreads();
  RZ_TS(2);
  // 3. vertical pass: item = (output row, group of 4 columns)
  const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(pyr + (size_t)img * D.pyr_bytes + D.dst_off), (short)0, D.dw * D.dh, 0x00020000);
#pragma unroll
  for (int k = 0; k < kVIt; k++) {
    const int it = tid + k * BS;
    const int i = it / (kRzTW / 4), g = it - i * (kRzTW / 4);
    if (i >= ny || 4 * g >= nx) continue;
    const ResizeY y = yv[k];
    // (b * h) >> 16 as v_mul_hi_u32_u24(b << 8, h << 8): both factors stay below 2^24 (b <= 2048,
    // 0 <= h <= 32640), so the full-rate 24-bit high multiply gives the same bits as the
    // quarter-rate v_mul_hi_u32(b << 16, h); h << 8 comes straight out of its packed pair (v_perm)
    const uint32_t B0 = (uint32_t)y.b0 << 8, B1 = (uint32_t)y.b1 << 8;
    const uint2 p0 = *(const uint2*)&hb[(y.sy0 - ry0) * kRzTW + 4 * g];
    const uint2 p1 = *(const uint2*)&hb[(y.sy1 - ry0) * kRzTW + 4 * g];
    constexpr uint32_t kLo = 0x0C01000Cu, kHi = 0x0C03020Cu;  // bytes 0-1 / 2-3 -> bits 8..23
    const uint32_t h0[4] = {__builtin_amdgcn_perm(0u, p0.x, kLo), __builtin_amdgcn_perm(0u, p0.x, kHi),
                            __builtin_amdgcn_perm(0u, p0.y, kLo), __builtin_amdgcn_perm(0u, p0.y, kHi)};
    const uint32_t h1[4] = {__builtin_amdgcn_perm(0u, p1.x, kLo), __builtin_amdgcn_perm(0u, p1.x, kHi),
                            __builtin_amdgcn_perm(0u, p1.y, kLo), __builtin_amdgcn_perm(0u, p1.y, kHi)};
    auto mulhi24 = [](uint32_t x, uint32_t z) {
      return (uint32_t)(((uint64_t)(x & 0xFFFFFFu) * (z & 0xFFFFFFu)) >> 32);
    };
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t v = (mulhi24(B0, h0[j]) + mulhi24(B1, h1[j]) + 2) >> 2;
      packed |= v << (8 * j);
    }
    const int o = (oy0 + i) * D.dw + ox0 + 4 * g;
    if (4 * g + 4 <= nx) {
      __builtin_amdgcn_raw_buffer_store_b32(packed, rd, o, 0, 0);
    } else {
      for (int j = 0; j < nx - 4 * g; j++) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(packed >> (8 * j)), rd, o + j, 0, 0);
    }
  }
  RZ_TS(3);
#ifdef ORBX_RZ_PROBE
  __builtin_amdgcn_s_waitcnt(0);  // the stores have left
#endif
  RZ_TS(4);
  RZ_PROBE_WRITE(ts1 - ts0, ts2 - ts1, ts3 - ts2, ts4 - ts3, 0);
}

// f(0) && f(1) && ... && f(N - 1) with the index a compile-time constant: an unrolled loop that stops
// at the first false, whatever N is
template <class F, int... I>
__device__ __forceinline__ void unrolled_while(std::integer_sequence<int, I...>, F&& f) {
  (void)(f(std::integral_constant<int, I>{}) && ...);
}

// The fast path of a level (chosen at plan time, strip_resize_ok in plan.hip; every level of a 1.2
// pyramid takes it).  Same arithmetic, one barrier, no row sums through LDS: a block stages the
// footprint of a 256 x kRsTH output tile as k_resize does, at the compile-time stride kRsStride, and
// then each wave owns one strip of kRsR output rows: lane = 4 adjacent output columns.  The wave
// walks down the strip's source rows once, in order (each output row reads rows sy0, sy0 + 1, and
// sy0 advances by 1 or 2 per output row: the walk is wave-uniform, its row coefficients scalars).
//   per source row and lane: 3 aligned LDS dwords cover the 8 bytes from the group's first sx0
//   (sx1(last) - sx0(first) <= 7); two v_alignbyte put them at byte 0, one v_perm per column with a
//   per-lane selector pairs (S[sx0], S[sx1]) as u16, one v_dot2_u32_u16 against (a0, a1) gives
//   x = S0*a0 + S1*a1, and x & ~15 is ((x >> 4) << 4), the form the vertical multiply takes.
//   The previous and the current row's four values stay in registers; the next row's dwords are
//   read from LDS ahead of the arithmetic on the current one.
//   per output row: ((b0*h0) >> 16) + ((b1*h1) >> 16) + 2) >> 2 with
//   v_mul_hi_u32_u24(b << 12, h << 4) = (b*h) >> 16 (b <= 2048, h <= 32640: both factors below
//   2^24), four pixels packed into one dword store at (scalar row offset, per-lane column).
__global__ __launch_bounds__(BS) void k_resize_strip(ResizeDesc D, const uint8_t* __restrict__ in, size_t in_pitch,
                                                     uint8_t* __restrict__ pyr) {
  // (one row and 16 B more than the footprint: the read-ahead past a strip's last row and the third
  // dword of a row's last group stay inside the array; what they fetch is never selected)
  __shared__ __align__(16) uint8_t tin[(kRsRows + 1) * kRsStride + 16];
  RZ_TS(0);
  const int3 bi = xcd_block3(D.rm);
  const int img = bi.z, tid = threadIdx.x;
  const int2 fx = D.sbx[bi.x], fy = D.sby[bi.y];
  const int ox0 = bi.x * kRsTW, oy0 = bi.y * kRsTH;
  const int cx0 = fx.x, span = fx.y - cx0 + 1;
  const int ry0 = fy.x, nrows = fy.y - ry0 + 1;
  const uint8_t* const src0 = in + (size_t)img * in_pitch;
  const uint8_t* const srcl = pyr + (size_t)img * D.pyr_bytes + D.src_off;
  const uint8_t* src = D.src_off < 0 ? src0 : srcl;
  const int swh = D.sw * D.sh;
  // this lane's four columns and this wave's rows: their coefficients load beside the footprint
  const int strip = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = ox0 + 4 * (tid & 63);
  const int oys = oy0 + strip * kRsR;
  const int ni = min(kRsR, D.dh - oys);  // output rows of this wave (<= 0: none)
  ResizeX xc[4];
#pragma unroll
  for (int k = 0; k < 4; k++) xc[k] = D.X[min(c0 + k, D.dw - 1)];
  ResizeY yv[kRsR];
#pragma unroll
  for (int i = 0; i < kRsR; i++) yv[i] = D.Y[min(oys + i, D.dh - 1)];
  // 1. footprint -> LDS: item = (row, 16-B chunk) over the kRsStride / 16 chunks of a row (a
  //    compile-time division), all of a thread's chunk loads issued before their stores
  {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, (short)0, swh, 0x00020000);
    const int nch = (span + 15) >> 4;
    constexpr int kCh = kRsStride / 16;
    constexpr int kLd = (kRsRows * kCh + BS - 1) / BS;
    uint4 v[kLd];
#pragma unroll
    for (int u = 0; u < kLd; u++) {
      const int q = tid + u * BS;
      const int r = q / kCh, c = q - r * kCh;
      const int o = (ry0 + r) * D.sw + cx0 + 16 * c;
      v[u] = make_uint4(0, 0, 0, 0);
      if (r < nrows && c < nch) {
        if (o + 16 <= swh) {
          const auto t = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0);
          v[u] = make_uint4(t[0], t[1], t[2], t[3]);
        } else {  // last bytes of the level: byte loads, each range-checked (outside -> 0, never used)
          uint32_t w4[4] = {0, 0, 0, 0};
#pragma unroll
          for (int b = 0; b < 16; b++)
            w4[b >> 2] |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, o + b, 0, 0) << (8 * (b & 3));
          v[u] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kLd; u++) {
      const int q = tid + u * BS;
      const int r = q / kCh, c = q - r * kCh;
      if (r < nrows && c < nch) *(uint4*)&tin[r * kRsStride + 16 * c] = v[u];
    }
  }
  __syncthreads();
  RZ_TS(1);
  if (ni <= 0) return;  // (wave-uniform; no barrier follows)
  // 2. per-lane constants: the window's LDS position, a byte selector and a coefficient pair per column
  const int s0 = xc[0].sx0 - cx0;
  const uint32_t sh0 = (uint32_t)s0 & 3u;
  uint32_t sel[4];
  u16x2 aa[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    sel[k] = 0x0C000C00u | (uint32_t)(xc[k].sx0 - xc[0].sx0) | ((uint32_t)(xc[k].sx1 - xc[0].sx0) << 16);
    aa[k] = u16x2{(unsigned short)xc[k].a0, (unsigned short)xc[k].a1};
  }
  auto mulhi24 = [](uint32_t x, uint32_t z) {
    return (uint32_t)(((uint64_t)(x & 0xFFFFFFu) * (z & 0xFFFFFFu)) >> 32);
  };
  const uint8_t* p = tin + (yv[0].sy0 - ry0) * kRsStride + (s0 & ~3);
  uint32_t w[3], hp[4] = {0, 0, 0, 0}, hc[4];
  auto fetch = [&]() {  // the row at p -> w, p to the next row
    const uint32_t* q = (const uint32_t*)p;
    w[0] = q[0], w[1] = q[1], w[2] = q[2];
    p += kRsStride;
  };
  auto advance = [&]() {  // hp <- hc <- the horizontal pass of the fetched row; the next row's fetch goes out
    const uint32_t lo = __builtin_amdgcn_alignbyte(w[1], w[0], sh0);
    const uint32_t hi = __builtin_amdgcn_alignbyte(w[2], w[1], sh0);
    fetch();
#pragma unroll
    for (int k = 0; k < 4; k++) {
      hp[k] = hc[k];
      const uint32_t pr = __builtin_amdgcn_perm(hi, lo, sel[k]);
      hc[k] = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, pr), aa[k], 0u, false) & ~15u;
    }
  };
  const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(pyr + (size_t)img * D.pyr_bytes + D.dst_off), (short)0, D.dw * D.dh, 0x00020000);
  const int nv = D.dw - c0;  // valid columns of this lane's group (>= 4: all)
  fetch();
#pragma unroll
  for (int k = 0; k < 4; k++) hc[k] = 0;
  advance();  // hc = row sy0 of the strip's first output row
  int cur = yv[0].sy0;
  // (a fold over the row indices, not a loop: every yv[i] stays a named scalar whatever kRsR is)
  unrolled_while(std::make_integer_sequence<int, kRsR>{}, [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    if (i >= ni) return false;
    advance();
    cur++;
    if (cur < yv[i].sy1) {  // sy0 moved by 2
      advance();
      cur++;
    }
    const uint32_t B0 = (uint32_t)yv[i].b0 << 12, B1 = (uint32_t)yv[i].b1 << 12;
    uint32_t t[4];
#pragma unroll
    for (int k = 0; k < 4; k++) t[k] = mulhi24(B0, hp[k]) + mulhi24(B1, hc[k]) + 2;
    // t <= 1022: two sums per register, both halves >> 2 at once, then the four low bytes
    const uint32_t t01 = ((t[0] | (t[1] << 16)) >> 2) & 0x00FF00FFu, t23 = ((t[2] | (t[3] << 16)) >> 2) & 0x00FF00FFu;
    const uint32_t packed = __builtin_amdgcn_perm(t23, t01, 0x06040200u);
    const int orow = (oys + i) * D.dw;
    if (nv >= 4) {
      __builtin_amdgcn_raw_buffer_store_b32(packed, rd, c0, orow, 0);
    } else {
      for (int j = 0; j < nv; j++) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(packed >> (8 * j)), rd, c0 + j, orow, 0);
    }
    return true;
  });
  RZ_TS(2);
#ifdef ORBX_RZ_PROBE
  __builtin_amdgcn_s_waitcnt(0);  // the stores have left
#endif
  RZ_TS(3);
  RZ_PROBE_WRITE(ts1 - ts0, 0, ts2 - ts1, ts3 - ts2, 1);
}

// ----------------------------------------------------------------- blur
// GaussianBlur(7x7, sigma=2, BORDER_REFLECT_101), OpenCV 3.2 8U fixed point:
// integer kernel {k0..k6} (x256), exact integer row+column sums, then
// rint(acc/65536) on SIMD column groups (x < w&~3) and (acc+2^15)>>16 on the
// scalar tail; saturate to u8 (the integer kernel {18,34,49,55,49,34,18} sums to 257).  128x128 output tile per block, staged in LDS.
__constant__ int c_gauss[7];

__device__ __forceinline__ int reflect101(int p, int n) {
  if (n == 1) return 0;
  while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}

// Tile of kBlurTileW x kBlurTileH (128 x 128) outputs per 256-thread block.
// Input tile col 0 = x0-4 so that every 4-output group reads 3 aligned LDS
// dwords.  The tile arrives as 16-B buffer loads at the (unaligned) source row
// positions, stored to 16-B aligned LDS rows (rows reflected per row index;
// the <= 3 reflected columns each side are patched from LDS afterwards).
// Thread = 4 columns x a 16-row strip: row sums (byte dot products) go into a
// 7-row register window that slides down the strip; the column taps are exact
// packed-f32 FMAs on the row sums with the weights pre-scaled by 2^-16 (every
// partial sum is an integer multiple of 2^-16 below 2^8, exact in f32), rounded
// by the 1.5*2^23 add and packed by byte permutes: ~10 VALU per output (18.6
// with per-column byte aligns, v_rndne / v_med3 / v_cvt_pk_u8 per output; the
// kernel is VALU-issue-bound).  A strip's 16 packed output dwords stay in
// registers until the whole tile is done, then go through the (no longer
// needed) input tile in LDS in the tiled blurred-level order (8x16-B tiles)
// (chunks swizzled so that neither side has a bank conflict, see the write-out)
// and out as whole 128-B tiles of b128 stores.  7 waves per SIMD: 72 VGPRs,
// no scratch (8 spills 12 B per lane for the same time, profiles/r04/ab_blur_tiled.txt).
constexpr int kBIn = kBlurTileW + 16;  // input tile row stride (bytes, 16-B multiple)
constexpr int kBStrip = 16;            // output rows per thread
#ifndef ORBX_BLUR_WPE
#define ORBX_BLUR_WPE 7
#endif
__global__ __launch_bounds__(BS, ORBX_BLUR_WPE) void k_blur(const Geometry* __restrict__ G, const int* __restrict__ tile_level,
                                                            BatchPtrs B, XcdRemap R) {
  constexpr int TR = kBlurTileH + 6;
  __shared__ __align__(16) uint8_t tin[(TR + 1) * kBIn];
  const int2 bi = xcd_block2(R);
  const int tile = bi.x, img = bi.y, tid = threadIdx.x;
  const int l = tile_level[tile];
  const LevelGeom& L = G->lv[l];
  const int t = tile - L.tile_begin;
  const int x0 = (t % L.tiles_x) * kBlurTileW, y0 = (t / L.tiles_x) * kBlurTileH;
  const uint8_t* src = level_ptr(*G, B, img, l);
  uint8_t* dst = B.blur + (size_t)img * G->blur_bytes + L.boff;
  const int w = L.w, h = L.h, bs = L.bstride;
  // input tile rows y0-3 .. y0+H+2 (REFLECT_101), cols x0-4 .. x0+W+11
  {
    constexpr int CPR = kBIn / 16, NQ = TR * CPR, KQ = (NQ + BS - 1) / BS;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, (short)0, w * h, 0x00020000);
    uint32_t v[KQ][4];
    // only what an output of the level reads is staged: tile rows up to the last output row's + 3
    // and chunks that begin at or left of column w + 2, the right reflection's reach (the rest
    // would be reflected re-reads; what is computed from the unstaged LDS bytes lands in the
    // level's padding)
    const int ty_last = min(kBlurTileH, h - y0) + 5, j_last = (w + 2 - (x0 - 4)) >> 4;
#pragma unroll
    for (int k = 0; k < KQ; k++) {
      const int q = k * BS + tid;
      const int ty = q / CPR, j = q - ty * CPR;
      v[k][0] = v[k][1] = v[k][2] = v[k][3] = 0;
      if (q < NQ && ty <= ty_last && j <= j_last) {
        const int sy = reflect101(y0 - 3 + ty, h);
        const int o = sy * w + x0 - 4 + 16 * j;
        if (o >= 0 && o + 16 <= w * h) {
          const auto r = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0);
          v[k][0] = r[0];
          v[k][1] = r[1];
          v[k][2] = r[2];
          v[k][3] = r[3];
        } else {
          // a chunk straddling the level's first or last byte (a range check covers the whole
          // 16-B access): byte loads, each range-checked on its own (outside -> 0, patched below)
#pragma unroll
          for (int b = 0; b < 16; b++)
            v[k][b >> 2] |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, o + b, 0, 0) << (8 * (b & 3));
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KQ; k++) {
      const int q = k * BS + tid;
      const int ty = q / CPR, j = q - ty * CPR;
      if (q < NQ && ty <= ty_last && j <= j_last)
        *(uint4*)&tin[ty * kBIn + 16 * j] = make_uint4(v[k][0], v[k][1], v[k][2], v[k][3]);
    }
  }
  const bool left = x0 < 3, right = x0 + kBlurTileW + 3 > w;
  if (left || right) {
    // patch the reflected columns x in [-3, -1] and [w, w+2] of every tile row (read after a barrier:
    // the source columns are inside the row and were stored by other threads)
    __syncthreads();
    // two-phase (read all, then write) so no patched byte feeds another patch
    const int nfix = TR * 6;
    uint8_t vals[(TR * 6 + BS - 1) / BS];
#pragma unroll
    for (int k = 0; k < (TR * 6 + BS - 1) / BS; k++) {
      const int q = k * BS + tid;
      vals[k] = 0;
      if (q < nfix) {
        const int ty = q / 6, s = q - ty * 6;
        const int x = s < 3 ? -3 + s : w + (s - 3);
        const int c = x - (x0 - 4);
        if (c >= 0 && c < kBIn && (s < 3 ? left : right)) vals[k] = tin[ty * kBIn + reflect101(x, w) - (x0 - 4)];
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (TR * 6 + BS - 1) / BS; k++) {
      const int q = k * BS + tid;
      if (q < nfix) {
        const int ty = q / 6, s = q - ty * 6;
        const int x = s < 3 ? -3 + s : w + (s - 3);
        const int c = x - (x0 - 4);
        if (c >= 0 && c < kBIn && (s < 3 ? left : right)) tin[ty * kBIn + c] = vals[k];
      }
    }
  }
  __syncthreads();
  const int g = tid & (kBlurTileW / 4 - 1);
  const int ys = (tid / (kBlurTileW / 4)) * kBStrip;  // strip's first output row in the tile
  const int xg = x0 + 4 * g;
  // (threads past the level compute nothing but stay for the barriers of the tile write-out)
  const bool active = xg < w && y0 + ys < h;
  uint32_t outv[kBStrip];
  const uint32_t k0 = c_gauss[0], k1 = c_gauss[1], k2 = c_gauss[2], k3 = c_gauss[3];
  // horizontal taps as byte dot products (exact integers, weights < 256) straight on the three
  // aligned dwords [a b c] = tile bytes 4g .. 4g+11: output col j of the group takes bytes
  // j+1 .. j+7, i.e. ten v_dot4_u32_u8 with the taps pre-shifted into the word each byte sits in
  // (no byte-align step).  The accumulator starts at 0x4B000000, so the sum comes out as the f32
  // bits of 2^23 + s (s <= 257*255 < 2^23) and one packed subtract per two columns converts it.
  auto W4 = [](uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) { return b0 | b1 << 8 | b2 << 16 | b3 << 24; };
  const uint32_t wa0 = W4(0, k0, k1, k2), wb0 = W4(k3, k2, k1, k0);
  const uint32_t wa1 = W4(0, 0, k0, k1), wb1 = W4(k2, k3, k2, k1), wc1 = W4(k0, 0, 0, 0);
  const uint32_t wa2 = W4(0, 0, 0, k0), wb2 = W4(k1, k2, k3, k2), wc2 = W4(k1, k0, 0, 0);
  const uint32_t wb3 = W4(k0, k1, k2, k3), wc3 = W4(k2, k1, k0, 0);
  const float f0 = (float)k0 * (1.f / 65536.f), f1 = (float)k1 * (1.f / 65536.f), f2 = (float)k2 * (1.f / 65536.f),
              f3 = (float)k3 * (1.f / 65536.f);
  const float2v F0 = {f0, f0}, F1 = {f1, f1}, F2 = {f2, f2}, F3 = {f3, f3};
  const float2v two23 = {8388608.0f, 8388608.0f}, magic = {12582912.0f, 12582912.0f};
  // row sums (<= 257*255, exact in f32) of output cols xg..xg+3 on tile row ty, as two f32 pairs
  auto rowsum = [&](int ty, float2v (&o)[2]) {
    const uint32_t* r32 = (const uint32_t*)&tin[ty * kBIn + 4 * g];
    const uint32_t a = r32[0], b = r32[1], c = r32[2];
    constexpr uint32_t bias = 0x4B000000u;  // f32 2^23
    const uint32_t s0 = __builtin_amdgcn_udot4(b, wb0, __builtin_amdgcn_udot4(a, wa0, bias, false), false);
    const uint32_t s1 = __builtin_amdgcn_udot4(
        c, wc1, __builtin_amdgcn_udot4(b, wb1, __builtin_amdgcn_udot4(a, wa1, bias, false), false), false);
    const uint32_t s2 = __builtin_amdgcn_udot4(
        c, wc2, __builtin_amdgcn_udot4(b, wb2, __builtin_amdgcn_udot4(a, wa2, bias, false), false), false);
    const uint32_t s3 = __builtin_amdgcn_udot4(c, wc3, __builtin_amdgcn_udot4(b, wb3, bias, false), false);
    o[0] = (float2v){__uint_as_float(s0), __uint_as_float(s1)} - two23;
    o[1] = (float2v){__uint_as_float(s2), __uint_as_float(s3)} - two23;
  };
  // 7-row ring indexed by compile-time (r + i) % 7 in the unrolled loop: no register moves
  float2v win[7][2];
  if (active) {
#pragma unroll
  for (int r = 0; r < 6; r++) rowsum(ys + r, win[r]);
  const int simd_w = w & ~3;
  const bool all_simd = xg + 3 < simd_w;  // the whole group takes the SSE2 rounding
  // wave-uniform: the per-row tail fix-up below is a scalar branch (no exec-mask juggling per row)
  const bool wave_tail = __builtin_amdgcn_ballot_w64(!all_simd) != 0;

#pragma unroll
  for (int r = 0; r < kBStrip; r++) {
    rowsum(ys + r + 6, win[(r + 6) % 7]);
    // column taps on packed f32 pairs, each element exactly the scalar chain
    // fma(f3, w3, fma(f2, w2+w4, fma(f1, w1+w5, f0*(w0+w6)))) = acc / 2^16 (integer sums below
    // 2^24 scaled by a power of two); + 1.5*2^23 rounds it half-to-even (the SSE2 groups'
    // rint), leaving the integer in the low bits
    float2v acc[2];
    uint32_t rb[4];
#pragma unroll
    for (int hh = 0; hh < 2; hh++) {
      const float2v w0 = win[r % 7][hh], w1 = win[(r + 1) % 7][hh], w2 = win[(r + 2) % 7][hh],
                    w3 = win[(r + 3) % 7][hh], w4 = win[(r + 4) % 7][hh], w5 = win[(r + 5) % 7][hh],
                    w6 = win[(r + 6) % 7][hh];
      acc[hh] = __builtin_elementwise_fma(
          F3, w3, __builtin_elementwise_fma(F2, w2 + w4, __builtin_elementwise_fma(F1, w1 + w5, F0 * (w0 + w6))));
      const float2v rr = acc[hh] + magic;
      rb[2 * hh] = __float_as_uint(rr.x);
      rb[2 * hh + 1] = __float_as_uint(rr.y);
    }
    // low halves as u16 pairs, saturated to 255 (the kernel sums to 257), then the low bytes
    u16x2 p01 = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(rb[1], rb[0], 0x05040100u));
    u16x2 p23 = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(rb[3], rb[2], 0x05040100u));
    const u16x2 cap = {255, 255};
    p01 = __builtin_elementwise_min(p01, cap);
    p23 = __builtin_elementwise_min(p23, cap);
    uint32_t packed = __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, p23), __builtin_bit_cast(uint32_t, p01), 0x06040200u);
    if (wave_tail) {
      // the row's scalar tail (x >= w & ~3): (acc + 2^15) >> 16, selected per lane and column
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float aj = j == 0 ? acc[0].x : j == 1 ? acc[0].y : j == 2 ? acc[1].x : acc[1].y;
        const int v = min(((int)(aj * 65536.f) + (1 << 15)) >> 16, 255);
        const uint32_t fixed = (packed & ~(0xFFu << (8 * j))) | ((uint32_t)v << (8 * j));
        packed = xg + j >= simd_w ? fixed : packed;
      }
    }
    outv[r] = packed;
  }
  }  // active
  // Write-out in the level's tile layout (8 rows x 16 bytes = 128-B tiles, the layout k_describe
  // gathers from): the outputs go to LDS (the input tile is no longer read) in tile order, then
  // leave as whole 128-B lines, 16 B per lane: the block's 128 x 128 outputs are 16 tile rows of
  // 8 consecutive tiles (1 KB each).  Columns past w and rows past h land in the level's padding.
  //
  // LDS staging layout: 16-B chunk q = tile * 8 + row (tile = (yr >> 3) * 8 + tc, tc = g >> 2 the
  // tile column, row = yr & 7) sits at chunk  q ^ tc  = tile * 8 + (row ^ tc), not at q.  Why:
  //  - ds_write_b32 is served in 2 groups of 32 lanes, bank = dword address mod 32.  A group is one
  //    output row yr with g = 0..31, dword g & 3 of chunk (.. + tc) * 8 + row.  Unswizzled, all 8 tile
  //    columns land on the 4 banks row * 4 .. + 3 (8 addresses per bank: 16 LDS cycles instead of
  //    4, SQ_LDS_BANK_CONFLICT 177 per wave).  With row ^ tc the 8 tile columns take 8 different
  //    chunks mod 8, so the 32 lanes cover all 32 banks once.
  //  - ds_read_b128 is served in 4 groups of 16 lanes ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the
  //    same + 32), bank = dword address mod 64, i.e. chunk mod 16.  Lane = 8 * tl + row reads chunk
  //    (tile << 3) | (row ^ tl) with tile & 7 = tl, so chunk mod 16 = (tl & 1) << 3 | (row ^ tl):
  //    lanes 0-3 -> 0-3, 12-15 -> 12-15, 20-23 -> 4-7, 24-27 -> 8-11; lanes 4-7 -> 4-7, 8-11 ->
  //    8-11, 16-19 -> 0-3, 28-31 -> 12-15; the upper half likewise (tl ^ 4 permutes the low two
  //    bits' quads).  Every group covers the 16 chunk positions once, as the linear layout did.
  // The swizzle permutes chunks inside a tile only; the staging area keeps its size.
  __syncthreads();
  if (active) {
    // byte address of (row 0, this thread's dword): bits 4-6 hold the chunk, xor-ed per row below
    const int tc = g >> 2;
    const int a0 = ((ys >> 3) * (kBlurTileW / 16) + tc) * 128 + (tc & 7) * 16 + (g & 3) * 4;
#pragma unroll
    for (int r = 0; r < kBStrip; r++)
      *(uint32_t*)&tin[(a0 ^ ((r & 7) * 16)) + (r >> 3) * (kBlurTileW / 16) * 128] = outv[r];
  }
  __syncthreads();
  {
    const int ntx = bs >> 4, nty = (h + 7) >> 3;
    const int tx0 = x0 >> 4, ty0 = y0 >> 3;
    const __amdgpu_buffer_rsrc_t rd =
        __builtin_amdgcn_make_buffer_rsrc((void*)dst, (short)0, nty * ntx * 128, 0x00020000);
    constexpr int kTiles = (kBlurTileW / 16) * (kBlurTileH / 8), kChunks = kTiles * 8;  // 16-B chunks
#pragma unroll
    for (int k = 0; k < kChunks / BS; k++) {
      const int q = tid + k * BS, t = q >> 3, tr = t / (kBlurTileW / 16), tc = t - tr * (kBlurTileW / 16);
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 v = *(const u32x4*)&tin[(q ^ (tc & 7)) * 16];  // the staging swizzle, undone
      if (tx0 + tc < ntx && ty0 + tr < nty)
        __builtin_amdgcn_raw_buffer_store_b128(v, rd, (uint32_t)(((ty0 + tr) * ntx + tx0 + tc) * 128 + (q & 7) * 16), 0, 0);
    }
  }
}

// ------------------------------------------------------------------- FAST
// One wavefront per kFastCPW (2) FAST cell windows, one after the other (block = 1 wave); the next
// cell's window loads are issued before the current cell's work (0.733 -> 0.726 ms per step against
// one cell per wave, profiles/r04/ab_fast_cells_per_wave.txt).
// cv::FAST(window, th, nonmax) semantics (OpenCV 3.2 FAST_t<16>): a pixel of
// the detection region is a corner at threshold t iff >= 9 contiguous ring
// pixels are all > v+t or all < v-t; its cornerScore<16> S satisfies
// corner_t <=> S >= t, so one score map serves both thresholds.  NMS is strict
// against the 8 neighbours inside the region (0 outside).  The cell runs FAST at
// iniThFAST; only if nothing survives does it run again at minThFAST (a
// wave-uniform second pass, src/ORBextractor.cc:892-900).  Survivors are written
// in row-major order.
//
// The kernel is VALU-issue-bound, so every phase is shaped for few vector
// instructions per pixel:
//   1. window -> LDS: 16-B buffer loads at the (unaligned) row positions land on
//      16-B aligned LDS rows of compile-time stride S, so every ring / map
//      access below is an LDS read with an immediate offset (no address VALU);
//   2. compass quick test (two adjacent of ring pixels 0,4,8,12 beyond t), as
//      min(max(p0,p8), max(p4,p12)) > c+t or max(min(p0,p8), min(p4,p12)) < c-t
//      (six min/max on the raw bytes; 0.855 -> 0.820 ms against the earlier packed
//      sign-bit form), on TWO rows of a column per lane: the sub-steps u and u + 1 of a trip sit in
//      the low and high 16 bits of each register (ds_read_u8 x 2 + v_perm per byte pair), so the
//      six min/max, the two differences and their maximum are nine v_pk_*_{u,i}16 for 128
//      pixels; each half then has one SDWA compare against t whose scalar mask, and-ed with the
//      cell's column mask (one ballot per cell), is both the ballot and the branch condition.
//      Survivors are compacted by ballot rank as tile offsets e = y*S + x (the 7x7
//      neighbourhood's top-left), low half first, so the list stays row-major;
//   3. cornerScore and the corner test in ONE pass on the compacted list:
//      ring pixel p is packed as the f16 pair (1024+p, 1279-p) (one v_mad_i32_i24:
//      bits 0x6400+p / 0x64FF-p), the 9-arc maximum of both halves is two rounds
//      of v_pk_maximum3_f16 and the minimum over the 16 arcs three rounds of
//      v_pk_minimum3_f16, giving (min_k max_arc p, 255 - max_k min_arc p), so
//      S+1 = max(v - min_k max_arc p, max_k min_arc p - v) (= cornerScore<16> + 1)
//      and corner_t <=> S+1 > t; corners are compacted in place, the map holds S+1;
//   4. NMS at iniThFAST -> count (steps 2-3 ran at iniThFAST; an empty cell repeats
//      them at minThFAST); 5. NMS at the chosen threshold -> ballot-ranked row-major
//      writes.
constexpr int kMaxCell = 60;  // wCell,hCell <= 60 (checked on the host)

__device__ __forceinline__ uint32_t pk_max3_f16(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ uint32_t pk_min3_f16(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// cornerScore<16> + 1 of the pixel whose 7x7 neighbourhood starts at t (row stride S): the
// ring in OpenCV's makeOffsets order, offsets relative to the top-left (centre at 3S+3)
template <int S>
__device__ __forceinline__ int ring_score1(const uint8_t* t) {
  constexpr int o[16] = {6 * S + 3, 6 * S + 4, 5 * S + 5, 4 * S + 6, 3 * S + 6, 2 * S + 6, S + 5, 4,
                         3,         2,         S + 1,     2 * S,     3 * S,     4 * S,     5 * S + 1, 6 * S + 2};
  const int v = t[3 * S + 3];
  uint32_t P[16];
#pragma unroll
  for (int k = 0; k < 16; k++) P[k] = (uint32_t)((int)t[o[k]] * -65535 + 0x64FF6400);  // (0x64FF-p)<<16 | 0x6400+p
  uint32_t M3[16], M9[16];
#pragma unroll
  for (int k = 0; k < 16; k++) M3[k] = pk_max3_f16(P[k], P[(k + 1) & 15], P[(k + 2) & 15]);
#pragma unroll
  for (int k = 0; k < 16; k++) M9[k] = pk_max3_f16(M3[k], M3[(k + 3) & 15], M3[(k + 6) & 15]);
  const uint32_t a0 = pk_min3_f16(M9[0], M9[1], M9[2]), a1 = pk_min3_f16(M9[3], M9[4], M9[5]),
                 a2 = pk_min3_f16(M9[6], M9[7], M9[8]), a3 = pk_min3_f16(M9[9], M9[10], M9[11]),
                 a4 = pk_min3_f16(M9[12], M9[13], M9[14]);
  const uint32_t R = pk_min3_f16(pk_min3_f16(a0, a1, a2), pk_min3_f16(a3, a4, M9[15]), M9[15]);
  const int a = (v + 0x6400) - (int)(R & 0xFFFF);  // v - min_k max_arc p
  const int b = (0x64FF - v) - (int)(R >> 16);     // max_k min_arc p - v
  return max(a, b);
}

#ifdef ORBX_FAST_PROBE
// probe only: the necessary condition "4 contiguous of the 8 even ring points beyond t" (a 9-arc
// always holds 4 or 5 consecutive even positions), counted on the compass survivors
template <int S>
__device__ __forceinline__ bool even8_test(const uint8_t* t, int th) {
  constexpr int o[8] = {6 * S + 3, 5 * S + 5, 3 * S + 6, S + 5, 3, S + 1, 3 * S, 5 * S + 1};
  const int v = t[3 * S + 3];
  int p[8], lo2[8], hi2[8];
#pragma unroll
  for (int k = 0; k < 8; k++) p[k] = t[o[k]];
#pragma unroll
  for (int k = 0; k < 8; k++) lo2[k] = min(p[k], p[(k + 1) & 7]), hi2[k] = max(p[k], p[(k + 1) & 7]);
  int bl = 0, bh = 255;
#pragma unroll
  for (int k = 0; k < 8; k++) bl = max(bl, min(lo2[k], lo2[(k + 2) & 7])), bh = min(bh, max(hi2[k], hi2[(k + 2) & 7]));
  return bl > v + th || bh < v - th;
}
#endif

typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 as_s16x2(int v) { return __builtin_bit_cast(s16x2, v); }
__device__ __forceinline__ int as_int(s16x2 v) { return __builtin_bit_cast(int, v); }

__device__ __forceinline__ int lane_rank(uint64_t m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// two bytes as a 16-bit pair, packed where the bytes are loaded: left to itself the compiler packs
// them at their use, in a later block, where it no longer knows the loads zero-extended (a v_and per
// byte) and keeps both bytes live until then
__device__ __forceinline__ u16x2 pair16(uint8_t lo, uint8_t hi) {
  uint32_t v = __builtin_bit_cast(uint32_t, u16x2{lo, hi});
  asm("" : "+v"(v));
  return __builtin_bit_cast(u16x2, v);
}
// the lane mask of a condition as it stands in its scalar pair (__ballot goes through an integer
// compare, which materialises a condition that is not itself a compare: v_cndmask + v_cmp_ne)
__device__ __forceinline__ uint64_t ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// Phase probe (build with -DORBX_FAST_PROBE only; tools/fast_probe.py): per-phase s_memtime
// deltas of every cell wave, stored (plain vector stores, no contention) to a host-provided
// buffer of 8 words per wave, indexed img * ncells + cell.
#ifdef ORBX_FAST_PROBE
__device__ unsigned int* fast_probe_buf;
#define FAST_TS(k) const unsigned long long ts##k = __builtin_amdgcn_s_memtime()
#else
#define FAST_TS(k)
#endif

// S: LDS row stride of the window tile and the score map (multiple of 16, >= window width);
// RP: region rows per compass instruction (2 when the widest cell fits 32 lanes);
// NK: 16-B window loads per lane, enough for the launch group's tallest window (FastGroup::nk)
#ifndef ORBX_FAST_CPW
#define ORBX_FAST_CPW 2
#endif
constexpr int kFastCPW = ORBX_FAST_CPW;  // FAST cells per wave
template <int S, int RP, int NK>
__global__ __launch_bounds__(64) void k_fast(const Geometry* __restrict__ G, const CellInfo* __restrict__ cells,
                                             BatchPtrs B, int grp, XcdRemap R) {
  // dynamic LDS sized by the launch group's largest cell (G->fg[grp])
  extern __shared__ __align__(16) uint8_t fast_smem[];
  const int tile_bytes = G->fg[grp].tile_bytes, map_bytes = G->fg[grp].map_bytes;
  uint8_t* tile = fast_smem;
  uint8_t* smap = fast_smem + tile_bytes;
  uint16_t* list = (uint16_t*)(fast_smem + tile_bytes + map_bytes);
  const int2 bi = xcd_block2(R);
  const int img = bi.y, lane = threadIdx.x;
  // 1. window -> registers -> LDS: lane = (row, 16-B chunk); window pixel (r, col) lands at tile[r*S + col]
  constexpr int CPR = (S + 15) / 16, RPI = 64 / CPR;
  constexpr int KMAX = NK;  // the host sizes NK by the group's tallest window: NK * RPI >= its rows
  static_assert(NK >= 1 && NK <= (kMaxCell + 6 + RPI - 1) / RPI, "no window is taller than kMaxCell + 6 rows");
  const int lr = lane / CPR, lj = lane - lr * CPR;
  const bool lane_ok = lr < RPI;
  // every load unconditional (a lane outside the window reads past num_records and gets zeros): no
  // branch between them, so all KMAX are in flight before the first wait
  auto load_window = [&](const CellInfo& cc, uint32_t (&w)[KMAX][4]) {
    const uint8_t* lvl =
        cc.level == 0 ? B.in + (size_t)img * B.in_pitch : B.pyr + (size_t)img * G->pyr_bytes + cc.loff;
    const uint8_t* base = lvl + (size_t)(cc.y0 - 3) * cc.lw + (cc.x0 - 3);
    const int th = cc.y1 - cc.y0 + 7;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, th * cc.lw + S, 0x00020000);
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
      const int r = k * RPI + lr;
      const uint32_t off = (lane_ok && r < th) ? (uint32_t)(r * cc.lw + 16 * lj) : 0x80000000u;
      const auto q = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
      w[k][0] = q[0];
      w[k][1] = q[1];
      w[k][2] = q[2];
      w[k][3] = q[3];
    }
  };
  // kFastCPW cells per wave, one after another; the next cell's window loads are issued before the
  // current cell's work, so their latency hides behind it
  const int cell0 = G->fg[grp].c0 + bi.x * kFastCPW, cend = G->fg[grp].c1;
  CellInfo cn = cells[cell0];
  uint32_t vn[KMAX][4];
  load_window(cn, vn);
#pragma unroll
  for (int q = 0; q < kFastCPW; q++) {
  const int cell = cell0 + q;
  if (cell >= cend) break;  // wave-uniform
  const CellInfo c = cn;
  uint32_t v[KMAX][4];
#pragma unroll
  for (int k = 0; k < KMAX; k++)
#pragma unroll
    for (int e = 0; e < 4; e++) v[k][e] = vn[k][e];
  if (q + 1 < kFastCPW && cell + 1 < cend) {
    cn = cells[cell + 1];
    load_window(cn, vn);
  }
  const int W = c.x1 - c.x0 + 1, H = c.y1 - c.y0 + 1, TH = H + 6;
  FAST_TS(0);
  if (q > 0) __syncthreads();  // the previous cell's tile / map / list reads are done
  {
    // zero the score map (its border row/column stands for "outside the region")
    for (int i = lane * 16; i < map_bytes; i += 64 * 16) *(uint4*)(smap + i) = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
      const int r = k * RPI + lr;
      if (k * RPI < TH && lane_ok && r < TH) {
        if constexpr (S % 16 == 0) {
          *(uint4*)(tile + r * S + 16 * lj) = make_uint4(v[k][0], v[k][1], v[k][2], v[k][3]);
        } else {  // 8-B aligned rows: the chunk as two halves, the part past the stride dropped
          if (16 * lj + 8 <= S) *(uint2*)(tile + r * S + 16 * lj) = make_uint2(v[k][0], v[k][1]);
          if (16 * lj + 16 <= S) *(uint2*)(tile + r * S + 16 * lj + 8) = make_uint2(v[k][2], v[k][3]);
        }
      }
    }
  }
  __syncthreads();
  const int ini = min(max(G->ini_th, 0), 255), mint = min(max(G->min_th, 0), 255);
  const int ly = RP == 2 ? (lane >> 5) : 0, lx = RP == 2 ? (lane & 31) : lane;
  // the lanes whose column is inside the region (W only: once per cell), and those of them on a
  // compass instruction's first row
  const bool col_ok = lx < W, col_ok0 = col_ok && ly == 0;
  const uint64_t colm = ballot64(col_ok), colm0 = colm & 0xFFFFFFFFull;
  constexpr int QU = 8 / RP;
  static_assert(QU % 2 == 0, "the compass trip pairs its sub-steps");
#ifdef ORBX_FAST_PROBE
  unsigned long long ts_mid = 0;
  int n_compass = 0, n_even8 = 0, n_corner_ini = 0;
#endif
  // 2.+3. FAST(window, th): compass quick test at th, row-major compaction of tile offsets, then
  // cornerScore + the corner test at th on the compass list, corners compacted in place and their
  // S+1 written to the map (the score does not depend on th, so a second pass at another threshold
  // rewrites the same values).  Returns the corner count.
  auto detect = [&](int th) -> int {
    int n = 0;
    // QU * RP region rows per trip; nu: the sub-steps of the trip whose first row is inside the region
    // (wave-uniform).  Full trips (nu = QU) are branch-free; the peeled last trip skips the others.
    // Sub-steps u and u + 1 (RP rows apart: the same lane, the same column) share one set of
    // registers, u in the low and u + 1 in the high 16 bits, so the byte arithmetic of 128 pixels is
    // one packed 16-bit instruction; each half then has its own compare, ballot and row-major stores.
    auto trip = [&](int y0r, auto fullc, int nu) {
      constexpr bool full = decltype(fullc)::value;
      const int eb = (y0r + ly) * S + lx;
      u16x2 cv[QU / 2], c0[QU / 2], c4[QU / 2], c8[QU / 2], c12[QU / 2];
#pragma unroll
      for (int p = 0; p < QU / 2; p++) {
        if (!full && 2 * p >= nu) break;
        // an unpaired last sub-step reads its high half from rows past the window: at most three
        // rows, which lie in the score map behind the tile, and that half is never looked at
        const uint8_t* t = tile + eb + 2 * p * RP * S;
        const uint8_t* t2 = t + RP * S;
        cv[p] = pair16(t[3 * S + 3], t2[3 * S + 3]);
        c0[p] = pair16(t[6 * S + 3], t2[6 * S + 3]);
        c4[p] = pair16(t[3 * S + 6], t2[3 * S + 6]);
        c8[p] = pair16(t[3], t2[3]);
        c12[p] = pair16(t[3 * S], t2[3 * S]);
      }
#pragma unroll
      for (int p = 0; p < QU / 2; p++) {
        if (!full && 2 * p >= nu) break;
        // two ADJACENT compass points beyond the threshold <=> (p0 | p8) & (p4 | p12) per
        // polarity, i.e. min(max(p0,p8), max(p4,p12)) > c+t or max(min(p0,p8), min(p4,p12)) < c-t:
        // min/max on the raw bytes, one difference per polarity (within -255 .. 255)
        const u16x2 hi = __builtin_elementwise_min(__builtin_elementwise_max(c0[p], c8[p]),
                                                   __builtin_elementwise_max(c4[p], c12[p]));
        const u16x2 lo = __builtin_elementwise_max(__builtin_elementwise_min(c0[p], c8[p]),
                                                   __builtin_elementwise_min(c4[p], c12[p]));
        const s16x2 d = __builtin_elementwise_max(__builtin_bit_cast(s16x2, hi - cv[p]),
                                                  __builtin_bit_cast(s16x2, cv[p] - lo));  // > th <=> compass hit
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const int u = 2 * p + h;
          if (!full && u >= nu) break;
          // the hit mask is the compare's own scalar pair and-ed with the cell's lane mask, once as the
          // ballot and once as the branch condition (no vector instruction either way)
          const bool over = d[h] > th;
          const uint64_t overm = ballot64(over);  // taken beside the compare: in a later block it is rebuilt
          auto compact = [&](bool ok, uint64_t okm) {
            const uint64_t m = overm & okm;
            if (over && ok) list[n + lane_rank(m)] = (uint16_t)(eb + u * RP * S);
            n += __popcll(m);
          };
          // lane inside the region: every row of a full trip is; the peeled trip's last sub-step
          // may have only its first row inside (RP = 2, a wave-uniform branch)
          if (full || RP == 1 || y0r + u * RP + RP <= H) compact(col_ok, colm);
          else compact(col_ok0, colm0);
        }
      }
    };
    int y0r = 0;
    for (; y0r + QU * RP <= H; y0r += QU * RP) trip(y0r, std::true_type{}, QU);
    if (y0r < H) trip(y0r, std::false_type{}, (H - y0r + RP - 1) / RP);
    __syncthreads();
#ifdef ORBX_FAST_PROBE
    if (th == ini) ts_mid = __builtin_amdgcn_s_memtime(), n_compass = n;
#endif
    int nc = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      int e = 0, sc1 = 0;
      if (i < n) {
        e = list[i];
        sc1 = ring_score1<S>(tile + e);
      }
      // outside the branch, so the ballot is the compare's own mask (a flag set inside comes out
      // of it as a v_cndmask and goes into the ballot through a v_cmp_ne); an idle lane has sc1 = 0 <= th
      const bool corner = sc1 > th;
#ifdef ORBX_FAST_PROBE
      if (th == ini) n_even8 += __popcll(__ballot(i < n && even8_test<S>(tile + e, th)));
#endif
      const uint64_t m = __ballot(corner);
      __syncthreads();
      if (corner) {
        list[nc + lane_rank(m)] = (uint16_t)e;
        smap[e + S + 1] = (uint8_t)sc1;
      }
      nc += __popcll(m);
    }
    __syncthreads();
    return nc;
  };
  // strict NMS inside the region; the map's zero border stands for "outside"
  auto ring8_max = [&](int e) -> int {  // the largest of the eight neighbours' map values
    const uint8_t* m = smap + e;        // centre at m[S + 1]
    const int n0 = m[0], n1 = m[1], n2 = m[2], n3 = m[S], n4 = m[S + 2], n5 = m[2 * S], n6 = m[2 * S + 1],
              n7 = m[2 * S + 2];
    return max(max(max(n0, n1), max(n2, n3)), max(max(n4, n5), max(n6, n7)));
  };
  auto kept = [](int s, int mx, int thr) -> bool {  // thr = t + 1 in map units (S + 1)
    // a neighbour beats the centre iff nv >= thr and nv >= s, so with mx the largest of the eight the
    // centre stays iff s >= thr && s > 1 && !(mx >= max(thr, s)).  Where s >= thr that maximum is s,
    // which leaves s >= max(thr, 2) && s >= mx + 1: ONE compare, whose mask the ballots take as it is
    return s >= max(mx + 1, max(thr, 2));
  };
  auto keep = [&](int e, int thr) -> bool { return kept(smap[e + S + 1], ring8_max(e), thr); };
  // FAST at iniThFAST only (src/ORBextractor.cc:892): the map then holds exactly the corners at
  // iniThFAST, which is all NMS at iniThFAST looks at (a weaker neighbour never beats a centre)
  FAST_TS(1);
  int nc = detect(ini);
  FAST_TS(2);
#ifdef ORBX_FAST_PROBE
  n_corner_ini = nc;
#endif
  // 4. survivors at iniThFAST (verdict kept in bit 15 of the list entry)
  int cnt = 0;
  for (int i0 = 0; i0 < nc; i0 += 64) {
    const int i = i0 + lane;
    int e = 0, s = 0, mx = 0;
    if (i < nc) {
      e = list[i];
      s = smap[e + S + 1];
      mx = ring8_max(e);
    }
    // the verdict outside the branch, as in detect(): an idle lane has s = 0 and is not kept
    const bool k = kept(s, mx, ini + 1);
    const uint64_t km = ballot64(k);
    if (k) list[i] = (uint16_t)(e | 0x8000);
    cnt += __popcll(km);
  }
  // an empty cell runs FAST(window, minThFAST) (src/ORBextractor.cc:894-900): a wave-uniform
  // second pass, taken by ~10 % of the cells on the bench images
  FAST_TS(3);
  if (cnt == 0 && mint != ini) nc = detect(mint);
  FAST_TS(4);
  const int thr = (cnt > 0 ? ini : mint) + 1;
  // 5. row-major writes at the chosen threshold
  // survivor p goes to the cell's inline slot p (p < kin) or overflow slot p - kin (cell_slot)
  // (as one offset, no select between two pointers: the pointer select made the compiler give up
  // duplicating the cell loop, +7 % VALU per wave)
  uint32_t* const out = B.cand + (size_t)img * G->cand_total + c.ovf_off - c.kin;
  uint32_t* const out_in = B.cand + (size_t)img * G->cand_total + c.cand_off;
  const int kin = c.kin;
  int pos = 0;
  for (int i0 = 0; i0 < nc; i0 += 64) {
    const int i = i0 + lane;
    int e = 0;
    bool k = false;
    if (i < nc) {
      const int le = list[i];
      e = le & 0x7FFF;
      k = cnt > 0 ? (le >> 15) != 0 : keep(e, thr);  // at iniThFAST the verdict is already known
    }
    const uint64_t m = __ballot(k);
    if (k) {
      const int p = pos + lane_rank(m);
      const int y = e / S, x = e - y * S;
      if (p < c.cap)
      {
        const uint32_t v = ((uint32_t)(smap[e + S + 1] - 1) << 24) | ((uint32_t)(c.y0 + y) << 12) | (uint32_t)(c.x0 + x);
        if (p < kin) out_in[p]= v; else out[p] = v;
      }
    }
    pos += __popcll(m);
  }
  if (lane == 0) B.cell_count[(size_t)img * G->ncells + cell] = min(pos, c.cap);
#ifdef ORBX_FAST_PROBE
  FAST_TS(5);
  if (lane < 8 && fast_probe_buf) {
    // word 6: empty-cell flag | corners at iniThFAST << 1 | survivors at iniThFAST << 16;
    // word 7: compass survivors | even-8 survivors << 16 (both at iniThFAST)
    const unsigned long long t[8] = {ts1 - ts0, ts_mid - ts1, ts2 - ts_mid, ts3 - ts2, ts4 - ts3, ts5 - ts4,
                                     (unsigned long long)((cnt == 0) | (n_corner_ini << 1) | (cnt << 16)),
                                     (unsigned long long)(n_compass | (n_even8 << 16))};
    fast_probe_buf[((size_t)img * G->ncells + cell) * 8 + lane] = (unsigned int)t[lane];
  }
#endif
  }  // cells of this wave
}

// k_fast<S, RP, NK> for a launch group's load count nk = N0 or N0 + 1 (the plan refuses any other)
template <int S, int RP, int N0>
static auto fast_kernel(int nk) -> decltype(&k_fast<S, RP, N0>) {
  return nk <= N0 ? k_fast<S, RP, N0> : k_fast<S, RP, N0 + 1>;
}

// ----------------------------------------------------------------- octree
// One block per (level, image).  Restates DistributeOctTree as rounds over an
// explicit node list held in LDS (list order == the reference's std::list
// order): each round splits the selected nodes, pushes their non-empty
// children to the front (reversed, as successive push_front do) and keeps the
// rest in order.  Keypoints never move; each keeps the index of its node.
// Phase 2 sorts (size, creation sequence) descending -- the reference sorts
// by (size, heap pointer); DESIGN.md §Parity documents the tie-break.
struct OctSmem {
  int16_t* x0;  // [2*NC] double-buffered node list
  int16_t* y0;
  int16_t* x1;
  int16_t* y1;
  int* cnt;
  int* seq;
  int* ccnt;       // [NC*4]
  int16_t* cidx;   // [NC*4]
  int16_t* nidx;   // [NC]
  int* sa;         // [NC]
  int* sb;         // [NC]
  uint64_t* key;   // [NP2] (also best)
  int* cpre;       // [cell_cap+1]
  int* ctrl;       // [8]
  uint32_t* kp;    // [kcap] candidate positions
  uint16_t* kn;    // [kcap] candidate node | digit << 14
};

// octree block size NT per launch group (Geometry::og): the split rounds loop over every candidate
// of the level (thousands at levels 0-2: 512 threads there, 512 beat 256 for a single launch, 0.42
// -> 0.38 ms per 256 frames, and 1024 halved the resident blocks per CU, 0.71); the upper levels
// run as 256-thread blocks with a smaller LDS footprint, so more of them share a CU
// phase 2 sorts up to this many splittable nodes by rank (M^2 / NT compares per thread), more by
// the bitonic network
constexpr int kOctRankSortMax = 1024;

template <int NT>
__device__ __forceinline__ void bitonic_sort_desc(uint64_t* k, int n) {
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < n / 2; i += NT) {
        const int lo = 2 * i - (i & (stride - 1));
        const int hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const uint64_t a = k[lo], b = k[hi];
        if (desc ? (a < b) : (a > b)) {
          k[lo] = b;
          k[hi] = a;
        }
      }
      __syncthreads();
    }
  }
}

// Per-candidate state across the split rounds: the packed position (score<<24 |
// y<<12 | x, level-relative) and node | child digit<<14.  The first grp.kcap
// candidates of a level live in LDS for the whole kernel (sized on the host so
// the block still fits three per CU); only a level with more candidates keeps
// the rest in the global kpos/knode scratch.  Every round walks all candidates
// of the level, so keeping them out of memory removes the per-round L2/HBM
// round trips (counter traffic 240 -> ~100 MB per 512 images).
struct OctCands {
  uint32_t* lpos;
  uint16_t* lnd;
  int kcap;
  uint32_t* gpos;
  uint32_t* gnd;
  __device__ __forceinline__ uint32_t pos(int k) const { return k < kcap ? lpos[k] : gpos[k]; }
  __device__ __forceinline__ uint32_t nd(int k) const { return k < kcap ? (uint32_t)lnd[k] : gnd[k]; }
  __device__ __forceinline__ void set(int k, uint32_t p, uint32_t n) const {
    if (k < kcap) {
      lpos[k] = p;
      lnd[k] = (uint16_t)n;
    } else {
      gpos[k] = p;
      gnd[k] = n;
    }
  }
  __device__ __forceinline__ void set_nd(int k, uint32_t n) const {
    if (k < kcap) lnd[k] = (uint16_t)n; else gnd[k] = n;
  }
};

template <int NT, class F>
__device__ __forceinline__ void oct_cands(int T, const OctCands& c, F f) {
  for (int k = threadIdx.x; k < T; k += NT) {
    const uint32_t n0 = c.nd(k);
    uint32_t n = n0;
    f(k, c.pos(k), n);
    if (n != n0) c.set_nd(k, n);
  }
}

// Phase probe (build with -DORBX_OCT_PROBE only; tools/oct_probe.py): per block, s_memtime ticks
// of the path that finished the block: [0] the candidate pass before the rounds (pyramid path: the
// histogram and the sums above it; generic path: the load into LDS), [1] the roots, [2] / [3] the
// phase-1 rounds and their count, [4] / [5] phase 2's, [6] the path's total, [7] the level's
// candidate count, [8] the final pass (best response and output), [9] the path (1 pyramid, 2
// generic), [10] ticks spent on the pyramid path before the block left it for the generic one;
// kOctProbeWords words per block, indexed img * nlevels + l.
#ifdef ORBX_OCT_PROBE
constexpr int kOctProbeWords = 12;
__device__ unsigned int* oct_probe_buf;
#define OCT_TS(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#else
#define OCT_TS(v)
#endif

// The generic path: candidates held in LDS (or the global spill), every round walks them twice.  Any
// depth, any candidate count.  Returns the block's path: 0 (empty level) or 2.
template <int NT>
__device__ int oct_generic(const Geometry* __restrict__ G, const CellInfo* __restrict__ cells, const BatchPtrs& B,
                           const OctGroup& grp, unsigned char* smem_raw, int img, int l) {
  const int tid = threadIdx.x;
  const LevelGeom& L = G->lv[l];
  const int NC = grp.node_cap;
  const int NP2 = next_pow2(NC);
  OctSmem s;
  {
    unsigned char* p = smem_raw;
    s.x0 = (int16_t*)p; p += NC * 4;
    s.y0 = (int16_t*)p; p += NC * 4;
    s.x1 = (int16_t*)p; p += NC * 4;
    s.y1 = (int16_t*)p; p += NC * 4;
    s.cnt = (int*)p; p += NC * 8;
    s.seq = (int*)p; p += NC * 8;
    s.ccnt = (int*)p; p += NC * 16;
    s.cidx = (int16_t*)p; p += NC * 8;
    s.nidx = (int16_t*)p; p += NC * 2;
    s.sa = (int*)p; p += NC * 4;
    s.sb = (int*)p; p += NC * 4;
    p = (unsigned char*)(((uintptr_t)p + 7) & ~(uintptr_t)7);
    s.key = (uint64_t*)p; p += (size_t)NP2 * 8;
    s.cpre = (int*)p; p += (grp.cell_cap + 1) * 4;
    s.ctrl = (int*)p; p += 8 * 4;
    s.kp = (uint32_t*)p; p += (size_t)grp.kcap * 4;
    s.kn = (uint16_t*)p;
  }
  uint32_t* oct_out = B.oct + (size_t)img * G->oct_total + L.oct_off;
  int* oct_cnt = B.oct_count + (size_t)img * G->nlevels + l;
  const size_t kbase = (size_t)img * G->cand_total + L.cand_begin;
  OctCands oc{s.kp, s.kn, grp.kcap, B.kpos + kbase, (uint32_t*)B.knode + kbase};

  OCT_TS(ot0);
#ifdef ORBX_OCT_PROBE
  unsigned long long ot_p1 = 0, ot_p2 = 0;
  int n_p1 = 0, n_p2 = 0;
#endif
  // 1. candidates of this level in vToDistributeKeys order (cells row-major)
  const int ncl = L.cell_end - L.cell_begin;
  for (int c = tid; c < ncl; c += NT) s.cpre[c] = B.cell_count[(size_t)img * G->ncells + L.cell_begin + c];
  __syncthreads();
  const int T = block_exclusive_scan<NT>(s.cpre, ncl);
  if (tid == 0) s.cpre[ncl] = T;
  if (T == 0) {
    if (tid == 0) *oct_cnt = 0;
    return 0;
  }
  const int nIni = L.nIni;
  const float hX = L.hX;
  const int minBX = L.minBX, minBY = L.minBY;
  for (int i = tid; i < nIni; i += NT) s.ccnt[i] = 0;
  __syncthreads();
  const uint32_t* cand = B.cand + (size_t)img * G->cand_total;
  auto put_cand = [&](int k, uint32_t v) {
    const int xr = (int)(v & 0xFFF) - minBX, yr = (int)((v >> 12) & 0xFFF) - minBY;
    const uint32_t pos = (v & 0xFF000000u) | ((uint32_t)yr << 12) | (uint32_t)xr;
    int root = (int)((float)xr / hX);
    root = min(max(root, 0), nIni - 1);
    oc.set(k, pos, (uint32_t)root);
    atomicAdd(&s.ccnt[root], 1);
  };
  if (ncl >= NT / 2) {
    // many cells (the dense levels): one thread per cell walks its survivors (candidate
    // k = cpre[c] + i), four loads in flight at a time
    for (int c = tid; c < ncl; c += NT) {
      const int k0 = s.cpre[c], n = s.cpre[c + 1] - k0;
      const CellInfo& ci = cells[L.cell_begin + c];
      const int kin = ci.kin, off = ci.cand_off, ovf = ci.ovf_off - kin;  // slot i: i < kin ? off + i : ovf + i
      int i = 0;
      for (; i + 4 <= n; i += 4) {
        const uint32_t v0 = cand[(i < kin ? off : ovf) + i], v1 = cand[(i + 1 < kin ? off : ovf) + i + 1],
                       v2 = cand[(i + 2 < kin ? off : ovf) + i + 2], v3 = cand[(i + 3 < kin ? off : ovf) + i + 3];
        put_cand(k0 + i, v0);
        put_cand(k0 + i + 1, v1);
        put_cand(k0 + i + 2, v2);
        put_cand(k0 + i + 3, v3);
      }
      for (; i < n; i++) put_cand(k0 + i, cand[(i < kin ? off : ovf) + i]);
    }
  } else {
    // few cells with many survivors each: one thread per candidate, its cell by binary search
    for (int k = tid; k < T; k += NT) {
      int lo = 0, hi = ncl - 1;  // last c with cpre[c] <= k
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s.cpre[mid] <= k) lo = mid; else hi = mid - 1;
      }
      put_cand(k, cand[cell_slot(cells[L.cell_begin + lo], k - s.cpre[lo])]);
    }
  }
  __syncthreads();
  OCT_TS(ot1);
  // 2. roots -> list (empty roots erased, src/ORBextractor.cc:604-615)
  for (int i = tid; i < nIni; i += NT) s.sa[i] = s.ccnt[i] > 0 ? 1 : 0;
  __syncthreads();
  int S = block_exclusive_scan<NT>(s.sa, nIni);
  for (int i = tid; i < nIni; i += NT) {
    if (s.ccnt[i] > 0) {
      const int ni = s.sa[i];
      s.x0[ni] = (int16_t)(int)(hX * (float)i);
      s.x1[ni] = (int16_t)(int)(hX * (float)(i + 1));
      s.y0[ni] = 0;
      s.y1[ni] = (int16_t)(L.maxBY - minBY);
      s.cnt[ni] = s.ccnt[i];
      s.seq[ni] = i;
      s.nidx[i] = (int16_t)ni;
    }
  }
  __syncthreads();
  oct_cands<NT>(T, oc, [&](int, uint32_t, uint32_t& nd) { nd = (uint32_t)s.nidx[nd]; });
  // child counters of the next round are cleared by the pass that precedes that
  // round's opening barrier (here, and after each round's remap): one barrier
  // per round fewer than a separate clear
  for (int i = tid; i < S * 4; i += NT) s.ccnt[i] = 0;
  OCT_TS(ot2);
  int cur = 0;
  int seqBase = nIni;
  int phase = 1;
  const int N = L.nfeat;
  for (int round = 0; round < 256; round++) {
    __syncthreads();
#ifdef ORBX_OCT_PROBE
    const unsigned long long rt0 = __builtin_amdgcn_s_memtime();
    const int rphase = phase;
    struct RoundStamp {
      unsigned long long t0;
      int ph;
      unsigned long long *p1, *p2;
      int *n1, *n2;
      __device__ ~RoundStamp() {
        const unsigned long long d = __builtin_amdgcn_s_memtime() - t0;
        if (ph == 1) { *p1 += d; ++*n1; } else { *p2 += d; ++*n2; }
      }
    } rstamp{rt0, rphase, &ot_p1, &ot_p2, &n_p1, &n_p2};
#endif
    const int nb = cur ^ 1;
    // kp pass A: child digit of every keypoint whose node splits (count > 1)
    oct_cands<NT>(T, oc, [&](int, uint32_t v, uint32_t& nd) {
      const int n = (int)(nd & 0x3FFF);
      if ((s.cnt + cur * NC)[n] > 1) {
        const int nx0 = (s.x0 + cur * NC)[n], ny0 = (s.y0 + cur * NC)[n];
        const int hx = (int)__builtin_ceilf((float)((s.x1 + cur * NC)[n] - nx0) / 2);
        const int hy = (int)__builtin_ceilf((float)((s.y1 + cur * NC)[n] - ny0) / 2);
        const float fx = (float)(int)(v & 0xFFF), fy = (float)(int)((v >> 12) & 0xFFF);
        const int d = (fx < (float)(nx0 + hx) ? 0 : 1) + (fy < (float)(ny0 + hy) ? 0 : 2);
        nd = (uint32_t)n | ((uint32_t)d << 14);
        atomicAdd(&s.ccnt[n * 4 + d], 1);
      }
    });
    __syncthreads();
    int C, Snew;
    if (phase == 1) {
      // split every node with > 1 keypoint, in list order.  One scan of packed
      // (children | kept << 16 | expandable children << 32) gives each node its
      // child and kept positions and the round's totals.
      for (int i = tid; i < S; i += NT) {
        const bool split = (s.cnt + cur * NC)[i] > 1;
        uint64_t v = split ? 0 : (1ull << 16);
        if (split)
          for (int d = 0; d < 4; d++) {
            const int cc = s.ccnt[i * 4 + d];
            v += (cc > 0 ? 1ull : 0ull) + (cc > 1 ? (1ull << 32) : 0ull);
          }
        s.key[i] = v;
      }
      __syncthreads();
      const uint64_t tot = block_scan_excl<NT, uint64_t>(s.key, S);
      C = (int)(tot & 0xFFFF);
      const int Sg = (int)((tot >> 16) & 0xFFFF);
      const int nexp = (int)(tot >> 32);
      for (int i = tid; i < S; i += NT) {
        const uint64_t pre = s.key[i];
        if ((s.cnt + cur * NC)[i] > 1) {
          const int nx0 = (s.x0 + cur * NC)[i], ny0 = (s.y0 + cur * NC)[i], nx1 = (s.x1 + cur * NC)[i], ny1 = (s.y1 + cur * NC)[i];
          const int hx = (int)__builtin_ceilf((float)(nx1 - nx0) / 2);
          const int hy = (int)__builtin_ceilf((float)(ny1 - ny0) / 2);
          int rank = 0;
          for (int d = 0; d < 4; d++) {
            const int cc = s.ccnt[i * 4 + d];
            if (cc == 0) continue;
            const int p = (int)(pre & 0xFFFF) + rank++;
            const int ni = C - 1 - p;
            (s.x0 + nb * NC)[ni] = (int16_t)((d & 1) ? nx0 + hx : nx0);
            (s.x1 + nb * NC)[ni] = (int16_t)((d & 1) ? nx1 : nx0 + hx);
            (s.y0 + nb * NC)[ni] = (int16_t)((d & 2) ? ny0 + hy : ny0);
            (s.y1 + nb * NC)[ni] = (int16_t)((d & 2) ? ny1 : ny0 + hy);
            (s.cnt + nb * NC)[ni] = cc;
            (s.seq + nb * NC)[ni] = seqBase + p;
            s.cidx[i * 4 + d] = (int16_t)ni;
          }
        } else {
          const int ni = C + (int)((pre >> 16) & 0xFFFF);
          (s.x0 + nb * NC)[ni] = (s.x0 + cur * NC)[i];
          (s.x1 + nb * NC)[ni] = (s.x1 + cur * NC)[i];
          (s.y0 + nb * NC)[ni] = (s.y0 + cur * NC)[i];
          (s.y1 + nb * NC)[ni] = (s.y1 + cur * NC)[i];
          (s.cnt + nb * NC)[ni] = (s.cnt + cur * NC)[i];
          (s.seq + nb * NC)[ni] = (s.seq + cur * NC)[i];
          s.nidx[i] = (int16_t)ni;
        }
      }
      __syncthreads();  // children / cidx / nidx written before the candidates remap
      oct_cands<NT>(T, oc, [&](int, uint32_t, uint32_t& nd) {
        const int n = (int)(nd & 0x3FFF);
        nd = (uint32_t)((s.cnt + cur * NC)[n] > 1 ? s.cidx[n * 4 + (nd >> 14)] : s.nidx[n]);
      });
      Snew = C + Sg;
      for (int i = tid; i < Snew * 4; i += NT) s.ccnt[i] = 0;
      seqBase += C;
      const bool finish = Snew >= N || Snew == S;
      S = Snew;
      cur = nb;
      if (finish) break;
      if (Snew + 3 * nexp > N) phase = 2;
    } else {
      // phase 2: split the largest (size, seq) first until the list reaches N
      for (int i = tid; i < S; i += NT) s.sa[i] = (s.cnt + cur * NC)[i] > 1 ? 1 : 0;
      __syncthreads();
      const int M = block_exclusive_scan<NT>(s.sa, S);
      const int P2 = next_pow2(max(M, 2));
      for (int i = tid; i < P2; i += NT) s.key[i] = 0;
      __syncthreads();
      for (int i = tid; i < S; i += NT)
        if ((s.cnt + cur * NC)[i] > 1)
          s.key[s.sa[i]] = ((uint64_t)(s.cnt + cur * NC)[i] << 43) | ((uint64_t)(s.seq + cur * NC)[i] << 13) | (uint64_t)i;
      __syncthreads();
      if (M <= kOctRankSortMax) {
        // descending order by rank (keys are distinct: they carry the node index): key j goes to
        // #{keys > key j}; one pass over the M keys per key instead of log2(P2)^2/2 barrier stages
        uint64_t* tmp = reinterpret_cast<uint64_t*>(s.cidx);  // cidx is rewritten below
        for (int j = tid; j < M; j += NT) {
          const uint64_t x = s.key[j];
          int r = 0;
#pragma unroll 4
          for (int y = 0; y < M; y++) r += s.key[y] > x ? 1 : 0;
          tmp[r] = x;
        }
        __syncthreads();
        for (int j = tid; j < M; j += NT) s.key[j] = tmp[j];
        __syncthreads();
      } else {
        bitonic_sort_desc<NT>(s.key, P2);
      }
      if (tid == 0) s.ctrl[1] = M - 1;
      for (int j = tid; j < M; j += NT) {
        const int n = (int)(s.key[j] & 0x1FFF);
        int nc = 0;
        for (int d = 0; d < 4; d++) nc += s.ccnt[n * 4 + d] > 0;
        s.sb[j] = nc - 1;
      }
      __syncthreads();
      // inclusive prefix of growth; first j reaching N
      block_exclusive_scan<NT>(s.sb, M);  // exclusive
      for (int j = tid; j < M; j += NT) {
        const int n = (int)(s.key[j] & 0x1FFF);
        int nc = 0;
        for (int d = 0; d < 4; d++) nc += s.ccnt[n * 4 + d] > 0;
        if (S + s.sb[j] + (nc - 1) >= N) atomicMin(&s.ctrl[1], j);
      }
      __syncthreads();
      const int m = s.ctrl[1];
      // children positions in processing order j = 0..m
      for (int j = tid; j < M; j += NT) {
        int nc = 0;
        if (j <= m) {
          const int n = (int)(s.key[j] & 0x1FFF);
          for (int d = 0; d < 4; d++) nc += s.ccnt[n * 4 + d] > 0;
        }
        s.sb[j] = nc;
      }
      for (int i = tid; i < S; i += NT) s.nidx[i] = -1;  // -1: processed marker set below
      __syncthreads();
      C = block_exclusive_scan<NT>(s.sb, M);
      for (int j = tid; j <= m; j += NT) {
        const int n = (int)(s.key[j] & 0x1FFF);
        s.nidx[n] = -2;  // processed
      }
      __syncthreads();
      for (int i = tid; i < S; i += NT) s.sa[i] = s.nidx[i] == -2 ? 0 : 1;
      __syncthreads();
      const int rest = block_exclusive_scan<NT>(s.sa, S);
      for (int j = tid; j <= m; j += NT) {
        const int i = (int)(s.key[j] & 0x1FFF);
        const int nx0 = (s.x0 + cur * NC)[i], ny0 = (s.y0 + cur * NC)[i], nx1 = (s.x1 + cur * NC)[i], ny1 = (s.y1 + cur * NC)[i];
        const int hx = (int)__builtin_ceilf((float)(nx1 - nx0) / 2);
        const int hy = (int)__builtin_ceilf((float)(ny1 - ny0) / 2);
        int rank = 0;
        for (int d = 0; d < 4; d++) {
          const int cc = s.ccnt[i * 4 + d];
          if (cc == 0) continue;
          const int p = s.sb[j] + rank++;
          const int ni = C - 1 - p;
          (s.x0 + nb * NC)[ni] = (int16_t)((d & 1) ? nx0 + hx : nx0);
          (s.x1 + nb * NC)[ni] = (int16_t)((d & 1) ? nx1 : nx0 + hx);
          (s.y0 + nb * NC)[ni] = (int16_t)((d & 2) ? ny0 + hy : ny0);
          (s.y1 + nb * NC)[ni] = (int16_t)((d & 2) ? ny1 : ny0 + hy);
          (s.cnt + nb * NC)[ni] = cc;
          (s.seq + nb * NC)[ni] = seqBase + p;
          s.cidx[i * 4 + d] = (int16_t)ni;
        }
      }
      for (int i = tid; i < S; i += NT) {
        if (s.nidx[i] == -2) continue;
        const int ni = C + s.sa[i];
        (s.x0 + nb * NC)[ni] = (s.x0 + cur * NC)[i];
        (s.x1 + nb * NC)[ni] = (s.x1 + cur * NC)[i];
        (s.y0 + nb * NC)[ni] = (s.y0 + cur * NC)[i];
        (s.y1 + nb * NC)[ni] = (s.y1 + cur * NC)[i];
        (s.cnt + nb * NC)[ni] = (s.cnt + cur * NC)[i];
        (s.seq + nb * NC)[ni] = (s.seq + cur * NC)[i];
        s.nidx[i] = (int16_t)ni;
      }
      __syncthreads();
      oct_cands<NT>(T, oc, [&](int, uint32_t, uint32_t& nd) {
        const int n = (int)(nd & 0x3FFF);
        const int ni = s.nidx[n];  // -2: n was split this round
        nd = (uint32_t)(ni == -2 ? s.cidx[n * 4 + (nd >> 14)] : ni);
      });
      Snew = C + rest;
      for (int i = tid; i < Snew * 4; i += NT) s.ccnt[i] = 0;
      seqBase += C;
      const bool finish = Snew >= N || Snew == S;
      S = Snew;
      cur = nb;
      if (finish) break;
    }
  }
  __syncthreads();
  OCT_TS(otf);
  // 3. best response per node: max score, then lowest candidate index
  for (int i = tid; i < S; i += NT) s.key[i] = 0;
  __syncthreads();
  oct_cands<NT>(T, oc, [&](int k, uint32_t v, uint32_t& nd) {
    const uint32_t x = (v & 0xFFF) + minBX, y = ((v >> 12) & 0xFFF) + minBY;
    const uint64_t key = ((uint64_t)(v >> 24) << 56) | ((uint64_t)(0xFFFFFFu - (uint32_t)k) << 24) |
                         (uint64_t)((y << 12) | x);
    atomicMax((unsigned long long*)&s.key[nd & 0x3FFF], (unsigned long long)key);
  });
  __syncthreads();
  const int nout = min(S, L.oct_cap);
  for (int i = tid; i < nout; i += NT) {
    const uint64_t key = s.key[i];
    oct_out[i] = ((uint32_t)(key >> 56) << 24) | (uint32_t)(key & 0xFFFFFF);
  }
  if (tid == 0) *oct_cnt = nout;
#ifdef ORBX_OCT_PROBE
  if (tid == 0 && oct_probe_buf) {
    const unsigned long long ot3 = __builtin_amdgcn_s_memtime();
    unsigned int* o = oct_probe_buf + ((size_t)img * G->nlevels + l) * kOctProbeWords;
    o[0] = (unsigned int)(ot1 - ot0);
    o[1] = (unsigned int)(ot2 - ot1);
    o[2] = (unsigned int)ot_p1;
    o[3] = (unsigned int)n_p1;
    o[4] = (unsigned int)ot_p2;
    o[5] = (unsigned int)n_p2;
    o[6] = (unsigned int)(ot3 - ot0);
    o[7] = (unsigned int)T;
    o[8] = (unsigned int)(ot3 - otf);
    o[9] = 2;
  }
#endif
  return 2;
}

// ------------------------------------------------------ octree: the count-pyramid path
// DivideNode splits a box at x0 + ceil((x1 - x0) / 2), y0 + ceil((y1 - y0) / 2): the whole tree's
// geometry is fixed by the level's roots, and a candidate's child digits down to any depth are a
// function of its position and its root.  Everything the rounds decide (which nodes split, the
// children kept, nexp, the switch to phase 2, phase 2's (size, sequence) order, the stop conditions)
// depends on the candidates only through how many lie in each box.  So: ONE pass over the candidates
// counts them into the boxes of depth D, the counts of depths D - 1 .. 0 are summed from those, the
// rounds run on the node list alone (a node's children's counts are two dword reads), and one more
// pass hands each candidate to its final node for the best-response pick.  Two candidate passes,
// where the generic path takes two per round and three around them.
//
// A block leaves this path for the generic one (from the start; nothing has been written to global
// memory by then) when a round selects a node of depth D with more than one candidate for
// splitting, or when the level holds more candidates than a 16-bit counter counts.
// f(k, v) for candidate k = 0 .. T-1 of the level in vToDistributeKeys order (cells row-major), v its
// FAST slot; cpre: exclusive prefix of the level's cell counts, cpre[ncl] = T
template <int NT, class F>
__device__ __forceinline__ void oct_walk(const LevelGeom& L, const CellInfo* __restrict__ cells,
                                         const uint32_t* __restrict__ cand, const int* cpre, int T, F f) {
  const int tid = threadIdx.x, ncl = L.cell_end - L.cell_begin;
  if (ncl >= NT / 2) {
    // many cells: one thread per cell walks its survivors, four loads in flight at a time
    for (int c = tid; c < ncl; c += NT) {
      const int k0 = cpre[c], n = cpre[c + 1] - k0;
      const CellInfo& ci = cells[L.cell_begin + c];
      const int kin = ci.kin, off = ci.cand_off, ovf = ci.ovf_off - kin;  // slot i: i < kin ? off + i : ovf + i
      int i = 0;
      for (; i + 4 <= n; i += 4) {
        const uint32_t v0 = cand[(i < kin ? off : ovf) + i], v1 = cand[(i + 1 < kin ? off : ovf) + i + 1],
                       v2 = cand[(i + 2 < kin ? off : ovf) + i + 2], v3 = cand[(i + 3 < kin ? off : ovf) + i + 3];
        f(k0 + i, v0);
        f(k0 + i + 1, v1);
        f(k0 + i + 2, v2);
        f(k0 + i + 3, v3);
      }
      for (; i < n; i++) f(k0 + i, cand[(i < kin ? off : ovf) + i]);
    }
  } else {
    // few cells with many survivors each: one thread per candidate, its cell by binary search
    for (int k = tid; k < T; k += NT) {
      int lo = 0, hi = ncl - 1;  // last c with cpre[c] <= k
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cpre[mid] <= k) lo = mid; else hi = mid - 1;
      }
      f(k, cand[cell_slot(cells[L.cell_begin + lo], k - cpre[lo])]);
    }
  }
}

// Returns the block's path: 0 (empty level), 1 (done), 2 (nothing written: run the generic path).
template <int NT>
__device__ int oct_pyramid(const Geometry* __restrict__ G, const CellInfo* __restrict__ cells, const BatchPtrs& B,
                           const OctGroup& grp, int D, unsigned char* smem_raw, int img, int l) {
  const int tid = threadIdx.x;
  const LevelGeom& L = G->lv[l];
  const int NC = grp.node_cap;
  const int nIni = L.nIni;
  const OctPyrLayout lay = oct_pyr_layout(NC, grp.cell_cap, grp.pcap, grp.span, nIni, D);
  uint64_t* key = (uint64_t*)(smem_raw + lay.key);
  uint64_t* tmp = (uint64_t*)(smem_raw + lay.tmp);
  uint32_t* cell = (uint32_t*)(smem_raw + lay.cell);
  int* cnt = (int*)(smem_raw + lay.cnt);
  int* seq = (int*)(smem_raw + lay.seq);
  int* sa = (int*)(smem_raw + lay.sa);
  int* sb = (int*)(smem_raw + lay.sb);
  int* cpre = (int*)(smem_raw + lay.cpre);
  int* ctrl = (int*)(smem_raw + lay.ctrl);
  int16_t* nidx = (int16_t*)(smem_raw + lay.nidx);
  uint32_t* kp = (uint32_t*)(smem_raw + lay.kp);
  uint16_t* xtab = (uint16_t*)(smem_raw + lay.tab);
  uint32_t* pyrw = (uint32_t*)(smem_raw + lay.pyr);  // the counters as dwords (a pair each)
  uint16_t* pyr = (uint16_t*)(smem_raw + lay.pyr);
  uint32_t* oct_out = B.oct + (size_t)img * G->oct_total + L.oct_off;
  int* oct_cnt = B.oct_count + (size_t)img * G->nlevels + l;

  OCT_TS(ot0);
#ifdef ORBX_OCT_PROBE
  unsigned long long ot_p1 = 0, ot_p2 = 0;
  int n_p1 = 0, n_p2 = 0;
#endif
  // 1. the level's candidate count, and every box's
  const int ncl = L.cell_end - L.cell_begin;
  for (int c = tid; c < ncl; c += NT) cpre[c] = B.cell_count[(size_t)img * G->ncells + L.cell_begin + c];
  __syncthreads();
  const int T = block_exclusive_scan<NT>(cpre, ncl);
  if (tid == 0) cpre[ncl] = T;
  if (T == 0) {
    if (tid == 0) *oct_cnt = 0;
    return 0;
  }
  if (T > 0xFFFF) return 2;
  const float hX = L.hX;
  const int minBX = L.minBX, minBY = L.minBY, boxH = max(L.maxBY - minBY, 1);
  const int npw = (oct_pyr_counters(nIni, D) + 1) / 2;
  for (int i = tid; i < npw; i += NT) pyrw[i] = 0;
  if (tid == 0) ctrl[0] = 0;  // 1: a round selected a node of depth D
  const int boxW = max(L.maxBX - minBX, 1);
  uint16_t* ytab = xtab + boxW;
  for (int i = tid; i < boxW + boxH; i += NT) {
    int lo, hi, g = 0;
    const bool isx = i < boxW;
    const float f = (float)(isx ? i : i - boxW);
    if (isx) {
      g = (int)(f / hX);
      g = min(max(g, 0), nIni - 1);
      lo = (int)(hX * (float)g);
      hi = (int)(hX * (float)(g + 1));
    } else {
      lo = 0;
      hi = boxH;
    }
    for (int d = 0; d < D; d++) {
      const int h = (int)__builtin_ceilf((float)(hi - lo) / 2);
      const int q = f < (float)(lo + h) ? 0 : 1;
      if (q) lo += h; else hi = lo + h;
      g = 2 * g + q;
    }
    xtab[i] = (uint16_t)g;
  }
  __syncthreads();
  const uint32_t* cand = B.cand + (size_t)img * G->cand_total;
  const int offD = oct_pyr_off(nIni, D);
  // a candidate's box of depth D.  DivideNode halves x and y independently, and the root a candidate is
  // filed under is a function of its x: gx at depth D depends on the column alone, gy on the row
  // alone.  (xtab / ytab, filled above with the same arithmetic: the root as DistributeOctTree files
  // it, then D halvings.)
  auto leaf = [&](uint32_t v, int& gx, int& gy) {
    const int xr = (int)(v & 0xFFF) - minBX, yr = (int)((v >> 12) & 0xFFF) - minBY;
    gx = xtab[min(max(xr, 0), boxW - 1)];
    gy = ytab[min(max(yr, 0), boxH - 1)];
  };
  const int kcap = grp.pcap;
  oct_walk<NT>(L, cells, cand, cpre, T, [&](int k, uint32_t v) {
    int gx, gy;
    leaf(v, gx, gy);
    const int idx = offD + gy * (nIni << D) + gx;
    atomicAdd(&pyrw[idx >> 1], 1u << ((idx & 1) * 16));
    if (k < kcap) kp[k] = v;  // kept for the final pass when the whole level fits
  });
  __syncthreads();
  for (int d = D - 1; d >= 0; d--) {
    const int W = nIni << d, n = W << d, o = oct_pyr_off(nIni, d), oc = oct_pyr_off(nIni, d + 1);
    for (int c = tid; c < n; c += NT) {
      const int gy = c / W, gx = c - gy * W;
      const int ci = oc + 2 * gy * 2 * W + 2 * gx;  // children (2gx, 2gy), (2gx + 1, 2gy); the next row 2W on
      const uint32_t w0 = pyrw[ci >> 1], w1 = pyrw[(ci + 2 * W) >> 1];
      pyr[o + c] = (uint16_t)((w0 & 0xFFFF) + (w0 >> 16) + (w1 & 0xFFFF) + (w1 >> 16));
    }
    __syncthreads();
  }
  OCT_TS(ot1);
  // a node's box (d, gx, gy) as one word; its counter; its children's counts by digit
  auto slot = [&](uint32_t c) {
    const int d = (int)(c >> 28);
    return oct_pyr_off(nIni, d) + (int)((c >> 20) & 0xFF) * (nIni << d) + (int)(c & 0xFFFFF);
  };
  auto kids = [&](uint32_t c, int* cc) {
    const int d = (int)(c >> 28) + 1, W = nIni << d;
    const int ci = oct_pyr_off(nIni, d) + 2 * (int)((c >> 20) & 0xFF) * W + 2 * (int)(c & 0xFFFFF);
    const uint32_t w0 = pyrw[ci >> 1], w1 = pyrw[(ci + W) >> 1];
    cc[0] = (int)(w0 & 0xFFFF);
    cc[1] = (int)(w0 >> 16);
    cc[2] = (int)(w1 & 0xFFFF);
    cc[3] = (int)(w1 >> 16);
  };
  auto child = [&](uint32_t c, int q) {
    return (((c >> 28) + 1) << 28) | ((2 * ((c >> 20) & 0xFF) + (uint32_t)(q >> 1)) << 20) |
           (2 * (c & 0xFFFFF) + (uint32_t)(q & 1));
  };
  constexpr uint16_t kSplit = 0xFFFF;  // a split node's own counter: descend (node indices are < 8192)
  // 2. roots -> list (empty roots erased, src/ORBextractor.cc:604-615)
  for (int i = tid; i < nIni; i += NT) sa[i] = pyr[i] > 0 ? 1 : 0;
  __syncthreads();
  int S = block_exclusive_scan<NT>(sa, nIni);
  for (int i = tid; i < nIni; i += NT) {
    if (pyr[i] > 0) {
      const int ni = sa[i];
      cell[ni] = (uint32_t)i;
      cnt[ni] = pyr[i];
      seq[ni] = i;
    }
  }
  OCT_TS(ot2);
  int cur = 0;
  int seqBase = nIni;
  int phase = 1;
  const int N = L.nfeat;
  for (int round = 0; round < 256; round++) {
    __syncthreads();
#ifdef ORBX_OCT_PROBE
    const unsigned long long rt0 = __builtin_amdgcn_s_memtime();
    const int rphase = phase;
    struct RoundStamp {
      unsigned long long t0;
      int ph;
      unsigned long long *p1, *p2;
      int *n1, *n2;
      __device__ ~RoundStamp() {
        const unsigned long long d = __builtin_amdgcn_s_memtime() - t0;
        if (ph == 1) { *p1 += d; ++*n1; } else { *p2 += d; ++*n2; }
      }
    } rstamp{rt0, rphase, &ot_p1, &ot_p2, &n_p1, &n_p2};
#endif
    const int nb = cur ^ 1;
    const uint32_t* ccell = cell + cur * NC;
    const int *ccnt = cnt + cur * NC, *cseq = seq + cur * NC;
    uint32_t* ncell = cell + nb * NC;
    int *ncnt = cnt + nb * NC, *nseq = seq + nb * NC;
    int C, Snew;
    if (phase == 1) {
      // split every node with > 1 candidate, in list order.  One scan of packed
      // (children | kept << 16 | expandable children << 32) gives each node its
      // child and kept positions and the round's totals.
      for (int i = tid; i < S; i += NT) {
        uint64_t v = 1ull << 16;
        if (ccnt[i] > 1) {
          v = 0;
          if ((int)(ccell[i] >> 28) >= D) {
            ctrl[0] = 1;
          } else {
            int cc[4];
            kids(ccell[i], cc);
            for (int q = 0; q < 4; q++) v += (cc[q] > 0 ? 1ull : 0ull) + (cc[q] > 1 ? (1ull << 32) : 0ull);
          }
        }
        key[i] = v;
      }
      __syncthreads();
      if (ctrl[0]) return 2;
      const uint64_t tot = block_scan_excl<NT, uint64_t>(key, S);
      C = (int)(tot & 0xFFFF);
      const int Sg = (int)((tot >> 16) & 0xFFFF);
      const int nexp = (int)(tot >> 32);
      for (int i = tid; i < S; i += NT) {
        const uint64_t pre = key[i];
        if (ccnt[i] > 1) {
          const uint32_t c = ccell[i];
          int cc[4];
          kids(c, cc);
          int rank = 0;
          for (int q = 0; q < 4; q++) {
            if (cc[q] == 0) continue;
            const int p = (int)(pre & 0xFFFF) + rank++;
            const int ni = C - 1 - p;
            ncell[ni] = child(c, q);
            ncnt[ni] = cc[q];
            nseq[ni] = seqBase + p;
          }
          pyr[slot(c)] = kSplit;
        } else {
          const int ni = C + (int)((pre >> 16) & 0xFFFF);
          ncell[ni] = ccell[i];
          ncnt[ni] = ccnt[i];
          nseq[ni] = cseq[i];
        }
      }
      Snew = C + Sg;
      seqBase += C;
      const bool finish = Snew >= N || Snew == S;
      S = Snew;
      cur = nb;
      if (finish) break;
      if (Snew + 3 * nexp > N) phase = 2;
    } else {
      // phase 2: split the largest (size, seq) first until the list reaches N.  A node of depth D
      // counts as one child here (its children's counts are not held): the walk's stop m is then
      // either right or at or past that node, and a selected node of depth D ends this path.
      auto nchild = [&](int n) {
        if ((int)(ccell[n] >> 28) >= D) return 1;
        int cc[4];
        kids(ccell[n], cc);
        return (cc[0] > 0) + (cc[1] > 0) + (cc[2] > 0) + (cc[3] > 0);
      };
      for (int i = tid; i < S; i += NT) sa[i] = ccnt[i] > 1 ? 1 : 0;
      __syncthreads();
      const int M = block_exclusive_scan<NT>(sa, S);
      const int P2 = next_pow2(max(M, 2));
      for (int i = tid; i < P2; i += NT) key[i] = 0;
      __syncthreads();
      for (int i = tid; i < S; i += NT)
        if (ccnt[i] > 1) key[sa[i]] = ((uint64_t)ccnt[i] << 43) | ((uint64_t)cseq[i] << 13) | (uint64_t)i;
      __syncthreads();
      if (M <= kOctRankSortMax) {
        // descending order by rank (keys are distinct: they carry the node index): key j goes to
        // #{keys > key j}; one pass over the M keys per key instead of log2(P2)^2/2 barrier stages
        for (int j = tid; j < M; j += NT) {
          const uint64_t x = key[j];
          int r = 0;
#pragma unroll 4
          for (int y = 0; y < M; y++) r += key[y] > x ? 1 : 0;
          tmp[r] = x;
        }
        __syncthreads();
        for (int j = tid; j < M; j += NT) key[j] = tmp[j];
        __syncthreads();
      } else {
        bitonic_sort_desc<NT>(key, P2);
      }
      if (tid == 0) ctrl[1] = M - 1;
      for (int j = tid; j < M; j += NT) sb[j] = nchild((int)(key[j] & 0x1FFF)) - 1;
      __syncthreads();
      // inclusive prefix of growth; first j reaching N
      block_exclusive_scan<NT>(sb, M);  // exclusive
      for (int j = tid; j < M; j += NT) {
        const int nc = nchild((int)(key[j] & 0x1FFF));
        if (S + sb[j] + (nc - 1) >= N) atomicMin(&ctrl[1], j);
      }
      __syncthreads();
      const int m = ctrl[1];
      // children positions in processing order j = 0..m
      for (int j = tid; j < M; j += NT) {
        int nc = 0;
        if (j <= m) {
          const int n = (int)(key[j] & 0x1FFF);
          if ((int)(ccell[n] >> 28) >= D) ctrl[0] = 1;
          nc = nchild(n);
        }
        sb[j] = nc;
      }
      for (int i = tid; i < S; i += NT) nidx[i] = -1;  // -2: split this round, set below
      __syncthreads();
      if (ctrl[0]) return 2;
      C = block_exclusive_scan<NT>(sb, M);
      for (int j = tid; j <= m; j += NT) nidx[(int)(key[j] & 0x1FFF)] = -2;
      __syncthreads();
      for (int i = tid; i < S; i += NT) sa[i] = nidx[i] == -2 ? 0 : 1;
      __syncthreads();
      const int rest = block_exclusive_scan<NT>(sa, S);
      for (int j = tid; j <= m; j += NT) {
        const int i = (int)(key[j] & 0x1FFF);
        const uint32_t c = ccell[i];
        int cc[4];
        kids(c, cc);
        int rank = 0;
        for (int q = 0; q < 4; q++) {
          if (cc[q] == 0) continue;
          const int p = sb[j] + rank++;
          const int ni = C - 1 - p;
          ncell[ni] = child(c, q);
          ncnt[ni] = cc[q];
          nseq[ni] = seqBase + p;
        }
        pyr[slot(c)] = kSplit;
      }
      for (int i = tid; i < S; i += NT) {
        if (nidx[i] == -2) continue;
        const int ni = C + sa[i];
        ncell[ni] = ccell[i];
        ncnt[ni] = ccnt[i];
        nseq[ni] = cseq[i];
      }
      Snew = C + rest;
      seqBase += C;
      const bool finish = Snew >= N || Snew == S;
      S = Snew;
      cur = nb;
      if (finish) break;
    }
  }
  __syncthreads();
  OCT_TS(otf);
  // 3. every final node's list index into its own counter, then each candidate descends from its
  // root through the split boxes to the index; best response per node: max score, then lowest
  // candidate index
  for (int i = tid; i < S; i += NT) {
    key[i] = 0;
    pyr[slot((cell + cur * NC)[i])] = (uint16_t)i;
  }
  __syncthreads();
  // the box of depth d above a box of depth D is its coordinates shifted: the D + 1 counters on a
  // candidate's way down are read side by side, the first that is no split mark is its node
  auto hand_over = [&](int k, uint32_t v) {
    int gx, gy;
    leaf(v, gx, gy);
    uint32_t nd = kSplit;
#pragma unroll
    for (int d = kOctMaxDepth; d >= 0; d--) {
      if (d > D) continue;
      const uint32_t c = pyr[oct_pyr_off(nIni, d) + (gy >> (D - d)) * (nIni << d) + (gx >> (D - d))];
      nd = c != kSplit ? c : nd;  // the shallowest wins: below a listed node the counters are stale counts
    }
    const uint64_t kv = ((uint64_t)(v >> 24) << 56) | ((uint64_t)(0xFFFFFFu - (uint32_t)k) << 24) | (uint64_t)(v & 0xFFFFFF);
    if (nd < (uint32_t)S) atomicMax((unsigned long long*)&key[nd], (unsigned long long)kv);
  };
  if (T <= kcap) {
    for (int k = tid; k < T; k += NT) hand_over(k, kp[k]);
  } else {
    oct_walk<NT>(L, cells, cand, cpre, T, hand_over);
  }
  __syncthreads();
  const int nout = min(S, L.oct_cap);
  for (int i = tid; i < nout; i += NT) {
    const uint64_t kv = key[i];
    oct_out[i] = ((uint32_t)(kv >> 56) << 24) | (uint32_t)(kv & 0xFFFFFF);
  }
  if (tid == 0) *oct_cnt = nout;
#ifdef ORBX_OCT_PROBE
  if (tid == 0 && oct_probe_buf) {
    const unsigned long long ot3 = __builtin_amdgcn_s_memtime();
    unsigned int* o = oct_probe_buf + ((size_t)img * G->nlevels + l) * kOctProbeWords;
    o[0] = (unsigned int)(ot1 - ot0);
    o[1] = (unsigned int)(ot2 - ot1);
    o[2] = (unsigned int)ot_p1;
    o[3] = (unsigned int)n_p1;
    o[4] = (unsigned int)ot_p2;
    o[5] = (unsigned int)n_p2;
    o[6] = (unsigned int)(ot3 - ot0);
    o[7] = (unsigned int)T;
    o[8] = (unsigned int)(ot3 - otf);
    o[9] = 1;
  }
#endif
  return 1;
}

template <int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(6))) void k_octree(const Geometry* __restrict__ G, const CellInfo* __restrict__ cells,
                                               BatchPtrs B, OctGroup grp, int* __restrict__ path) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  // level-major grid (images fastest): every image's level-0 block (the longest) is dispatched
  // first and the short top levels last, so the kernel's tail is short blocks (longest first;
  // image-major order left one level-0 block per image until the end: 0.302 -> 0.232 ms per step)
  const int img = blockIdx.x, l = grp.l0 + blockIdx.y;
  OCT_TS(kt0);
  int p = 2;
  if (grp.depth > 0) p = oct_pyramid<NT>(G, cells, B, grp, grp.depth, smem_raw, img, l);
  if (p == 2) {
    __syncthreads();  // the two paths overlay the block's LDS
#ifdef ORBX_OCT_PROBE
    const unsigned long long kt1 = __builtin_amdgcn_s_memtime();
#endif
    p = oct_generic<NT>(G, cells, B, grp, smem_raw, img, l);
#ifdef ORBX_OCT_PROBE
    if (threadIdx.x == 0 && oct_probe_buf)
      oct_probe_buf[((size_t)img * G->nlevels + l) * kOctProbeWords + 10] = grp.depth > 0 ? (unsigned int)(kt1 - kt0) : 0;
#endif
  }
  if (path && threadIdx.x == 0) path[(size_t)img * G->nlevels + l] = p;
}

// --------------------------------------------------------------- describe
// One wave per keypoint: IC_Angle on the raw level (src/ORBextractor.cc:77-105),
// computeOrbDescriptor on the blurred level (:110-152), then the keypoint
// record in level-major output order with pt *= mvScaleFactor[l] (:1201-1207).
// Sum over the 64 lanes (all active), returned wave-uniform: DPP row_shr 1/2/4/8
// prefix sums leave each 16-lane row's total in its last lane, then four readlanes.
// (Integer adds: the order is immaterial.)
__device__ __forceinline__ int wave_sum_dpp(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);
  return __builtin_amdgcn_readlane(v, 15) + __builtin_amdgcn_readlane(v, 31) + __builtin_amdgcn_readlane(v, 47) +
         __builtin_amdgcn_readlane(v, 63);
}


// describe's blurred patch: rotated bit_pattern_31_ points stay within radius 18.39, so
// |row|, |col| <= 18 after cvRound: a 37 x 37 patch around the keypoint
constexpr int kPatchR = 18;
constexpr int kPatchRows = 2 * kPatchR + 1;  // 37
constexpr int kPS = 80;  // LDS row stride of the staged patches (bytes): 20 dwords, so the rotated
                         // samples' rows spread over the banks (a 64-B stride folds every 4th row)
// bytes per wave: the blurred patch + the descriptor words
constexpr int kDescLds = kPatchRows * kPS + 256;
// half-width hw(r) of patch row r = 0..36 (row offset r - 18) the rotated pattern can reach
struct PatchHW {
  int v[kPatchRows];
};
constexpr PatchHW kPatchHW = {{6,  8,  10, 11, 12, 13, 14, 15, 16, 16, 17, 17, 18, 18, 18, 18, 18, 18, 18,
                               18, 18, 18, 18, 18, 18, 17, 17, 16, 16, 15, 14, 13, 12, 11, 10, 8,  6}};
__constant__ PatchHW c_patch_hw = kPatchHW;
// describe patch slots: slot s -> (row << 2 | k-th chunk of the row's span), 2 / 3 / 4 slots per row
// (the most 16-B chunks the row's span covers over the 16 alignments), 124 slots, 0xFF past them.
// Order: the four lanes of a quad (slots 4i .. 4i+3) are four consecutive rows of one chunk index --
// 64 contiguous bytes of the tiled blurred level whenever they fall inside one 8-row tile, two
// lines otherwise (a row-major quad touches 3-4) -- chunk index by chunk index; the one row each
// chunk index has left over (37 / 37 / 33 / 17 rows) shares the last quad: 31 quads.
struct PatchSlots {
  uint8_t e[128];
};
constexpr int patch_row_chunks(int r) {  // most chunks [18+a-hw, 18+a+hw] covers over a = 0..15
  int m = 0;
  for (int a = 0; a < 16; a++) {
    const int n = ((kPatchR + a + kPatchHW.v[r]) >> 4) - ((kPatchR + a - kPatchHW.v[r]) >> 4) + 1;
    m = n > m ? n : m;
  }
  return m;
}
constexpr PatchSlots make_patch_slots() {
  PatchSlots t{};
  for (int s = 0; s < 128; s++) t.e[s] = 0xFF;
  int n = 0, nrest = 0;
  uint8_t rest[12] = {};
  for (int ch = 0; ch < 4; ch++) {
    int rows[kPatchRows] = {}, nr = 0;  // rows whose span can reach a ch-th chunk (one contiguous run)
    for (int r = 0; r < kPatchRows; r++)
      if (patch_row_chunks(r) > ch) rows[nr++] = r;
    for (int q = 0; q + 4 <= nr; q += 4)
      for (int i = 0; i < 4; i++) t.e[n++] = (uint8_t)(rows[q + i] << 2 | ch);
    for (int q = nr & ~3; q < nr; q++) rest[nrest++] = (uint8_t)(rows[q] << 2 | ch);
  }
  for (int i = 0; i < nrest; i++) t.e[n++] = rest[i];
  return t;
}
constexpr PatchSlots kPatchSlots = make_patch_slots();
static_assert(kPatchSlots.e[123] != 0xFF && kPatchSlots.e[124] == 0xFF, "124 patch slots: two loads per lane");
__constant__ PatchSlots c_patch_slot = kPatchSlots;
const uint8_t* patch_slot_table() { return kPatchSlots.e; }

#ifndef ORBX_DESC_K
#define ORBX_DESC_K 8
#endif
constexpr int kDescK = ORBX_DESC_K;  // keypoints per wave
static_assert(kDescK * 8 <= 64, "one descriptor dword per lane");

// f(std::integral_constant<int, 0>{}) ... f(<N-1>): compile-time lane indices in an unrolled loop
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}
__device__ __forceinline__ const uint8_t* lane_ptr(const uint8_t* p, int j) {
  const uint64_t a = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)a, j), hi = __builtin_amdgcn_readlane((uint32_t)(a >> 32), j);
  return (const uint8_t*)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ float lane_f(float v, int j) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}

// k_describe: IC_Angle (src/ORBextractor.cc:77-105), computeOrbDescriptor (:110-152) on the blurred
// level k_blur wrote (:1186-1190), and the keypoint record in level-major output order with
// pt *= mvScaleFactor[l] (:1201-1207).
//
// kDescK keypoints per wave (consecutive output indices):
//   1. lane j finds keypoint i0 + j's level and loads its octree entry and level record;
//   2. the IC_Angle boxes of all kDescK keypoints and the blurred patches of the first two are
//      issued together; the moments are wave sums per keypoint (v_dot4 on circle-masked 16-B rows);
//   3. fastAtan2 and the deterministic sin/cos run once, lane j for keypoint j;
//   4. per keypoint: the blurred patch (only the pixels a rotated pair can reach) -> LDS, the patch
//      two ahead issued, then the 256 rotated pairs with pair p in lane p & 63: ballot k =
//      descriptor bits 64k .. 64k+63, staged in LDS;
//   5. one coalesced store of the kDescK descriptors (lane = dword) and the keypoint records.
__global__ __launch_bounds__(BS) void k_describe(const Geometry* __restrict__ G, BatchPtrs B,
                                                 orbx_keypoint* __restrict__ kps, uint8_t* __restrict__ desc,
                                                 int32_t* __restrict__ counts, int kp_cap, XcdRemap R) {
  __shared__ __align__(16) uint8_t s_desc[BS / 64][kDescLds];
  const int2 bi = xcd_block2(R);
  const int img = bi.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i0 = __builtin_amdgcn_readfirstlane((bi.x * (BS / 64) + wv) * kDescK);
  const int nl = G->nlevels;
  // per-level counts as independent scalar loads
  const int* oc = B.oct_count + (size_t)img * nl;
  int cnt[kMaxLevelsPlan];
#pragma unroll
  for (int ll = 0; ll < kMaxLevelsPlan; ll++) cnt[ll] = ll < nl ? oc[ll] : 0;
  int total = 0;
#pragma unroll
  for (int ll = 0; ll < kMaxLevelsPlan; ll++) total += cnt[ll];
  if (bi.x == 0 && threadIdx.x == 0) counts[img] = total;
  // the rBRIEF pairs of this lane (p = lane + 64k), reused for every keypoint of the wave
  float4 pat[4];
#pragma unroll
  for (int k = 0; k < 4; k++) pat[k] = reinterpret_cast<const float4*>(c_pattern_f)[lane + 64 * k];
  if (i0 >= total) return;  // wave-uniform: the DPP sums below see a full wave
  const int nk = min(kDescK, total - i0);
  // 1. lane j: keypoint i0 + min(j, nk - 1) (lanes past nk repeat the last one; never written)
  const int i = i0 + min(lane, nk - 1);
  int l = 0, first = 0, acc = 0;
#pragma unroll
  for (int ll = 0; ll < kMaxLevelsPlan; ll++) {
    if (i >= acc) {  // last level whose start is <= i
      l = ll;
      first = acc;
    }
    acc += cnt[ll];
  }
  const LevelGeom& L = G->lv[l];
  const uint32_t v = B.oct[(size_t)img * G->oct_total + L.oct_off + (i - first)];
  const int w = L.w, h = L.h;
  const float lscale = L.scale, lsize = L.kp_size;
  const int x = v & 0xFFF, y = (v >> 12) & 0xFFF, score = v >> 24;
  const uint8_t* lvl = level_ptr(*G, B, img, l);
  // IC box origin (x - 15, y - 15); keypoints sit >= 19 px inside the level, so the box is too
  const uint8_t* icp = lvl + (size_t)(y - 15) * w + (x - 15);

  // 2. IC boxes of every keypoint, then the first two blurred patches
  const int r = lane >> 1, hh = lane & 1;
  uint32_t q[kDescK][4];
#pragma unroll
  for (int j = 0; j < kDescK; j++) {
    const int wj = __builtin_amdgcn_readlane(w, j);
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)lane_ptr(icp, j), (short)0, 31 * wj, 0x00020000);
    const uint32_t off = lane < 62 ? (uint32_t)(r * wj + 16 * hh) : 0x80000000u;
    const auto t = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
    q[j][0] = t[0];
    q[j][1] = t[1];
    q[j][2] = t[2];
    q[j][3] = t[3];
  }
  constexpr int kPatchLd = 2;  // 16-B loads per lane per patch
  // the blurred level's patch: rows y-18..y+18, 16-B chunks from the 16-aligned column x0
  const int bs = L.bstride;
  const int x0 = (x - kPatchR) & ~15;
  const uint8_t* pbl = B.blur + (size_t)img * G->blur_bytes + L.boff;  // the level's tiles
  constexpr int PS = kPS;
  const uint32_t corr_l = (uint32_t)(kPatchR * PS + (x - x0)) - (0x400000u * (uint32_t)PS + 0x4B400000u);
  // Only the blurred pixels a rotated pattern point can land on are loaded: a point of radius rho
  // rounds to (r, c) with (|r| - 1/2)^2 + (|c| - 1/2)^2 <= rho^2 <= 338 (the pattern's largest
  // rho^2), so row r needs |c| <= hw(r) (c_patch_hw; equal to the brute-force reach of the pattern
  // over all angles).  Each row's span [18+a-hw, 18+a+hw] (a = (x-18) & 15, patch column 0 = the
  // 16-aligned level column x0) covers 2-4 16-B chunks: slot s = lane + 64k is (row, k-th chunk of
  // its span) (c_patch_slot), 124 slots, 99-112 of them valid by a -- two 16-B loads per lane
  // instead of three, 25-33 % fewer bytes than the full 37 x 64.
  int srow[kPatchLd], skk[kPatchLd], shw[kPatchLd];
#pragma unroll
  for (int k = 0; k < kPatchLd; k++) {
    const int e = c_patch_slot.e[lane + 64 * k];
    srow[k] = e == 0xFF ? -1 : e >> 2;
    skk[k] = e & 3;
    shw[k] = c_patch_hw.v[e == 0xFF ? 0 : e >> 2];
  }
  uint32_t pv[2][kPatchLd][4];
  int pdst[2][kPatchLd];  // LDS byte offset of each loaded chunk (-1: none)
  auto load_patch = [&](int j, uint32_t (&dst)[kPatchLd][4], int (&dofs)[kPatchLd]) {
    const int bt8 = __builtin_amdgcn_readlane(bs, j) * 8, hj = __builtin_amdgcn_readlane(h, j);
    const int xj = __builtin_amdgcn_readlane(x, j), y0j = __builtin_amdgcn_readlane(y, j) - kPatchR;
    const int aj = (xj - kPatchR) & 15, tx0 = (xj - kPatchR) >> 4;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)lane_ptr(pbl, j), (short)0, ((hj + 7) >> 3) * bt8, 0x00020000);
#pragma unroll
    for (int k = 0; k < kPatchLd; k++) {
      // 16-B chunks at 16-aligned columns: each is one row of an 8 x 16 tile (blur_tile_off), so the
      // chunks of eight patch rows in a column share one 128-B line
      const int lo = (kPatchR + aj - shw[k]) >> 4, hi = (kPatchR + aj + shw[k]) >> 4;
      const int ch = lo + skk[k];
      const bool ok = srow[k] >= 0 && ch <= hi;
      const int yy = y0j + srow[k];
      const uint32_t off = ok ? (uint32_t)((yy >> 3) * bt8 + (tx0 + ch) * 128 + (yy & 7) * 16) : 0x80000000u;
      dofs[k] = ok ? srow[k] * kPS + 16 * ch : -1;
      const auto t = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
      dst[k][0] = t[0];
      dst[k][1] = t[1];
      dst[k][2] = t[2];
      dst[k][3] = t[3];
    }
  };
  load_patch(0, pv[0], pdst[0]);
  if (kDescK > 1) load_patch(1, pv[1], pdst[1]);
  // moments: lane (r, hh) holds the 16 bytes at columns 16hh .. 16hh + 15 of box row r, masked to
  // the circle; s0 = sum I, s1 = sum b * I, m01 = (r - 15) s0, m10 = s1 + (16hh - 15) s0 (integers:
  // exact in any order).  Keypoint j's sums land in lane j.
  int M01 = 0, M10 = 0;
  {
    const uint4 mk = c_icmask[lane];
    static_for<kDescK>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      const uint32_t I0 = q[j][0] & mk.x, I1 = q[j][1] & mk.y, I2 = q[j][2] & mk.z, I3 = q[j][3] & mk.w;
      uint32_t s0 = __builtin_amdgcn_udot4(I0, 0x01010101u, 0u, false);
      s0 = __builtin_amdgcn_udot4(I1, 0x01010101u, s0, false);
      s0 = __builtin_amdgcn_udot4(I2, 0x01010101u, s0, false);
      s0 = __builtin_amdgcn_udot4(I3, 0x01010101u, s0, false);
      uint32_t s1 = __builtin_amdgcn_udot4(I0, 0x03020100u, 0u, false);
      s1 = __builtin_amdgcn_udot4(I1, 0x07060504u, s1, false);
      s1 = __builtin_amdgcn_udot4(I2, 0x0B0A0908u, s1, false);
      s1 = __builtin_amdgcn_udot4(I3, 0x0F0E0D0Cu, s1, false);
      const int m01 = wave_sum_dpp((r - 15) * (int)s0);
      const int m10 = wave_sum_dpp((int)s1 + (16 * hh - 15) * (int)s0);
      M01 = lane == j ? m01 : M01;
      M10 = lane == j ? m10 : M10;
    });
  }
  // 3. orientation of keypoint j in lane j
  const float angle = fast_atan2((float)M01, (float)M10);
  const float factorPI = (float)(3.14159265358979323846 / 180.f);
  float sn, cs;
  sincos_det(angle * factorPI, c_sincos, &sn, &cs);

  const float2v magic = {12582912.0f, 12582912.0f};  // 1.5 * 2^23: round half to even

  // 4. per keypoint
  uint8_t* pb = s_desc[wv];
  // the descriptors' 64-bit words, staged per wave and stored by lane = dword at the end
  uint64_t* sdw = reinterpret_cast<uint64_t*>(s_desc[wv] + kDescLds - 256);
  static_for<kDescK>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    if (j >= nk) return;  // wave-uniform
    uint32_t (&cur)[kPatchLd][4] = pv[j & 1];
    int (&cdst)[kPatchLd] = pdst[j & 1];
#pragma unroll
    for (int k = 0; k < kPatchLd; k++)
      if (cdst[k] >= 0) *(uint4*)(pb + cdst[k]) = make_uint4(cur[k][0], cur[k][1], cur[k][2], cur[k][3]);
    if (j + 2 < kDescK && j + 2 < nk) load_patch(j + 2, cur, cdst);
    const uint32_t corr = __builtin_amdgcn_readlane(corr_l, j);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // rotated pattern point (px, py) -> patch pixel (18 + r, 18 + c) with
    //   r = cvRound(px*b + py*a), c = cvRound(px*a - py*b)    (src/ORBextractor.cc:119-125)
    // Both coordinates ride in packed-f32 lanes.  Each sum is rounded exactly as the scalar
    // expression (products, then the add / subtract); adding 1.5*2^23 rounds it to an integer
    // half-to-even (|sum| < 2^22), leaving 0x4B400000 + r in the bits.  A 24-bit mad on the raw
    // bits ((0x400000 + r) * kPS, low 24 bits sign-extended) plus a constant gives the offset.
    const float a = lane_f(cs, j), b = lane_f(sn, j);
    const float2v ba = {b, a}, ab = {a, b};
    static_for<4>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      int t[2];
#pragma unroll
      for (int e = 0; e < 2; e++) {
        const float px = e ? pat[k].z : pat[k].x, py = e ? pat[k].w : pat[k].y;
        const float2v P = (float2v){px, px} * ba;   // {px*b, px*a}
        const float2v Q = (float2v){py, -py} * ab;  // {py*a, -(py*b)}: negation is exact
        const float2v M = (P + Q) + magic;
        const uint32_t mr = __float_as_uint(M.x), mc = __float_as_uint(M.y);
        t[e] = pb[(uint32_t)__mul24((int)mr, kPS) + mc + corr];
      }
      // bits 64k .. 64k + 63 of the descriptor: every lane stores the same wave-uniform word
      sdw[4 * j + k] = __ballot(t[0] < t[1]);
    });
    // the next keypoint's patches overwrite these: every lane's reads come first
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  });
  // 5. output: descriptors (lane = dword) and keypoint records (lane = keypoint)
  const size_t o0 = (size_t)img * kp_cap + i0;
  if (lane < 8 * nk) reinterpret_cast<uint32_t*>(desc + o0 * 32)[lane] = reinterpret_cast<const uint32_t*>(sdw)[lane];
  if (lane < nk) {
    orbx_keypoint kp;
    float fx = (float)x, fy = (float)y;
    if (l != 0) {
      fx *= lscale;
      fy *= lscale;
    }
    kp.x = fx;
    kp.y = fy;
    kp.size = lsize;
    kp.angle = angle;
    kp.response = (float)score;
    kp.octave = l;
    kp.class_id = -1;
    kps[o0 + lane] = kp;
  }
}

// ------------------------------------------------------------------ launch
hipError_t upload_constants(const int* umax16, const int* gauss7) {
  uint32_t mask[64][4] = {};
  for (int lane = 0; lane < 62; lane++) {
    const int r = lane >> 1, h = lane & 1, v = r - 15, um = umax16[v < 0 ? -v : v];
    for (int b = 0; b < 16; b++) {
      const int u = 16 * h + b - 15;
      if (u <= 15 && u >= -um && u <= um) mask[lane][b >> 2] |= 0xFFu << (8 * (b & 3));
    }
  }
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_icmask), mask, sizeof(mask));
  if (e != hipSuccess) return e;
  return hipMemcpyToSymbol(HIP_SYMBOL(c_gauss), gauss7, 7 * sizeof(int));
}

// The blurred levels of n_img images (also ORBX_DBG_BLUR_LEVEL, which re-blurs the last batch)
hipError_t launch_blur(const Geometry& Gh, const Geometry* Gd, const int* tile_level, const BatchPtrs& B, int n_img,
                       hipStream_t st) {
  XcdRemap R;
  if (!make_xcd_remap(Gh.ntiles, n_img, 1, &R)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_blur, dim3(Gh.ntiles, n_img), dim3(BS), 0, st, Gd, tile_level, B, R);
  return hipGetLastError();
}

// k_octree over n_img images' candidates (also orbx_debug_octree_candidates, on supplied candidates).
// (Launch order of the groups measured flat.)  One or two images: all levels in one launch (the groups'
// launches would run one after the other with a few blocks each)
hipError_t launch_octree(const Geometry& Gh, const Geometry* Gd, const CellInfo* cells, const BatchPtrs& B, int n_img,
                         hipStream_t st, int* path, int depth_cap) {
  const bool one = n_img <= kOctOneLaunch;
  for (int gi = 0; gi < (one ? 1 : Gh.n_og); gi++) {
    OctGroup og = one ? Gh.og_all : Gh.og[gi];
    const size_t smem = octree_group_smem(og);  // the plan's, whatever the cap
    if (depth_cap >= 0) og.depth = min(og.depth, depth_cap);
    if (og.nt == 512)
      hipLaunchKernelGGL(k_octree<512>, dim3(n_img, og.l1 - og.l0), dim3(512), smem, st, Gd, cells, B, og, path);
    else
      hipLaunchKernelGGL(k_octree<256>, dim3(n_img, og.l1 - og.l0), dim3(256), smem, st, Gd, cells, B, og, path);
  }
  return hipPeekAtLastError();
}

hipError_t launch_extract_stages(const Geometry& Gh, const Geometry* Gd, const CellInfo* cells, const int* tile_level,
                                 const LaunchPlan& LP, const BatchPtrs& B, int n_img, orbx_keypoint* kps, uint8_t* desc,
                                 int32_t* counts, int kp_cap, hipStream_t st, StageTimer* T) {
  // every grid's block-remap constants first (the only launch data that depends on the batch size),
  // so a grid they cannot serve is refused before any stage timer opens
  const int nb = (Gh.max_kps + BS / 64 * kDescK - 1) / (BS / 64 * kDescK);  // kDescK keypoints per wave
  ResizeDesc rz[kMaxLevelsPlan];
  dim3 rz_grid[kMaxLevelsPlan], fast_grid[2];
  XcdRemap fast_rm[2], desc_rm;
  for (int l = 1; l < Gh.nlevels; l++) {
    const int tw = LP.rz[l].strip ? kRsTW : kRzTW, th = LP.rz[l].strip ? kRsTH : kRzTH;
    rz_grid[l] = dim3((Gh.lv[l].w + tw - 1) / tw, (Gh.lv[l].h + th - 1) / th, n_img);
    rz[l] = LP.rz[l];
#ifdef ORBX_RZ_PROBE
    rz[l].level = l;
    rz[l].probe_base = l == 1 ? 0 : rz[l - 1].probe_base + (int)(rz_grid[l - 1].x * rz_grid[l - 1].y * rz_grid[l - 1].z);
#endif
    if (!make_xcd_remap(rz_grid[l].x, rz_grid[l].y, rz_grid[l].z, &rz[l].rm)) return hipErrorInvalidValue;
  }
  for (int g = 0; g < Gh.n_fg; g++) {
    const Geometry::FastGroup& F = Gh.fg[g];
    if (F.c1 <= F.c0) continue;
    fast_grid[g] = dim3((F.c1 - F.c0 + kFastCPW - 1) / kFastCPW, n_img);
    if (!make_xcd_remap(fast_grid[g].x, fast_grid[g].y, 1, &fast_rm[g])) return hipErrorInvalidValue;
  }
  XcdRemap blur_rm;
  if (!make_xcd_remap(Gh.ntiles, n_img, 1, &blur_rm) || !make_xcd_remap(max(nb, 1), n_img, 1, &desc_rm))
    return hipErrorInvalidValue;
  for (int l = 1; l < Gh.nlevels; l++) {
    T->begin(st);
    if (rz[l].strip)
      hipLaunchKernelGGL(k_resize_strip, rz_grid[l], dim3(BS), 0, st, rz[l], B.in, B.in_pitch, B.pyr);
    else
      hipLaunchKernelGGL(k_resize, rz_grid[l], dim3(BS), (size_t)Gh.rz_rows * (Gh.rz_stride + 2 * kRzTW), st, rz[l], B.in,
                         B.in_pitch, B.pyr);
    T->end(ST_RESIZE, st);
  }
  if (Gh.ncells > 0) {
    T->begin(st);
    for (int g = 0; g < Gh.n_fg; g++) {
      const Geometry::FastGroup& F = Gh.fg[g];
      if (F.c1 <= F.c0) continue;
      // (S, RP, NK) as the plan's layout chose them: S = 48 and 80 hold cells wider than 32 (RP = 1)
      auto kf = F.s == 40   ? (F.rp == 2 ? fast_kernel<40, 2, 2>(F.nk) : fast_kernel<40, 1, 2>(F.nk))
                : F.s == 48 ? fast_kernel<48, 1, 2>(F.nk)
                            : fast_kernel<80, 1, 4>(F.nk);
      hipLaunchKernelGGL(kf, fast_grid[g], dim3(64), F.smem, st, Gd, cells, B, g, fast_rm[g]);
    }
    T->end(ST_FAST, st);
  } else {
    (void)hipMemsetAsync(B.oct_count, 0, sizeof(int) * Gh.nlevels * n_img, st);
  }
  {
    T->begin(st);
    hipLaunchKernelGGL(k_blur, dim3(Gh.ntiles, n_img), dim3(BS), 0, st, Gd, tile_level, B, blur_rm);
    T->end(ST_BLUR, st);
  }
  if (Gh.ncells > 0) {
    T->begin(st);
    (void)launch_octree(Gh, Gd, cells, B, n_img, st);  // its error, if any, is the hipGetLastError below
    T->end(ST_OCTREE, st);
  }
  T->begin(st);
  hipLaunchKernelGGL(k_describe, dim3(max(nb, 1), n_img), dim3(BS), 0, st, Gd, B, kps, desc, counts, kp_cap, desc_rm);
  T->end(ST_DESCRIBE, st);
  return hipGetLastError();
}

hipError_t octree_set_smem_limit(size_t bytes) {
  hipError_t e = hipFuncSetAttribute((const void*)k_octree<512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute((const void*)k_octree<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace orbx

#ifdef ORBX_OCT_PROBE
extern "C" int orbx_debug_oct_probe(void* d_buf) {  // device buffer of 8 u32 per (image, level) block, or NULL
  unsigned int* p = (unsigned int*)d_buf;
  return hipMemcpyToSymbol(HIP_SYMBOL(orbx::oct_probe_buf), &p, sizeof(p)) == hipSuccess ? 0 : -3;
}
#endif
#ifdef ORBX_RZ_PROBE
extern "C" int orbx_debug_rz_probe(void* d_buf, unsigned int blocks) {  // device buffer of 8 u32 per resize block, or NULL
  unsigned int* p = (unsigned int*)d_buf;
  if (hipMemcpyToSymbol(HIP_SYMBOL(orbx::rz_probe_cap), &blocks, sizeof(blocks)) != hipSuccess) return -3;
  return hipMemcpyToSymbol(HIP_SYMBOL(orbx::rz_probe_buf), &p, sizeof(p)) == hipSuccess ? 0 : -3;
}
#endif
#ifdef ORBX_FAST_PROBE
extern "C" int orbx_debug_fast_probe(void* d_buf) {  // device buffer of 8 u32 per cell wave, or NULL
  unsigned int* p = (unsigned int*)d_buf;
  return hipMemcpyToSymbol(HIP_SYMBOL(orbx::fast_probe_buf), &p, sizeof(p)) == hipSuccess ? 0 : -3;
}
#endif

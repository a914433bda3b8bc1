// orbx_device.h -- device-side numerics shared by the HIP kernels.
//
// Everything here is compiled with -ffp-contract=off: every float/double
// expression rounds exactly as written, so results equal the CPU restatement
// of the reference (oracle/) bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orbx {

constexpr int kHalfPatch = 15;      // HALF_PATCH_SIZE, src/ORBextractor.cc:73
constexpr int kEdgeThreshold = 19;  // EDGE_THRESHOLD, src/ORBextractor.cc:74
constexpr int kMaxLevels = 16;

// cvRound (SSE2 cvtss2si): round half to even.
// XCD-aware block order.  MI355X deals blocks round-robin over its 8 XCDs,
// each with a private L2, so neighbouring blocks -- cells, tiles, keypoints
// that read overlapping image rows -- would each pull the shared lines into a
// different L2.  xcd_block maps the hardware linear block id so that the
// blocks sharing an XCD take one contiguous range of the logical grid.
// Bijective for any grid size (q + 1 blocks for the first total % 8 groups);
// affects speed only, never results.
__device__ __forceinline__ int xcd_block(int hw, int total) {
  const int x = hw & 7, i = hw >> 3, q = total >> 3, r = total & 7;
  return x * q + min(x, r) + i;
}
// logical (x, y) of a 2-D grid, x fastest
// (unsigned divisions: the block-uniform quotients are scalar instruction sequences, and the signed
// forms' abs / sign fix-ups made them a large part of a short kernel's scalar work)
__device__ __forceinline__ int2 xcd_block2() {
  const unsigned gx = gridDim.x;
  const unsigned l = (unsigned)xcd_block(blockIdx.x + gx * blockIdx.y, gx * gridDim.y);
  const unsigned q = l / gx;
  return make_int2((int)(l - q * gx), (int)q);
}
// logical (x, y, z) of a 3-D grid, x fastest
__device__ __forceinline__ int3 xcd_block3() {
  const unsigned gx = gridDim.x, gy = gridDim.y;
  const unsigned l = (unsigned)xcd_block(blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z), gx * gy * gridDim.z);
  const unsigned q = l / gx, z = q / gy;
  return make_int3((int)(l - q * gx), (int)(q - z * gy), (int)z);
}

// The same two maps without run-time divisions, for kernels short enough that the two
// v_rcp / v_readfirstlane / s_mul_hi sequences of about 25 instructions each show: the grid's
// constants come from the host by value (make_xcd_remap, once per launch).
//   l / d  ==  mulhi(2l + 1, m) >> s   with m = ceil(2^(31+s) / d), e = m*d - 2^(31+s) in [0, d):
//   (2l+1) m / 2^(32+s) = (2l+1)/(2d) + (2l+1) e / (2d 2^(31+s)); the first term is l/d + 1/(2d),
//   whose fraction is at most 1 - 1/(2d), so the floor is l / d as long as the second term stays
//   below 1/(2d), i.e. (2l+1) e < 2^(31+s).  make_xcd_remap takes the smallest s for which that
//   holds for every l < total with m below 2^32 (d = 1: m = 2^31, s = 0).  Needs total <= 2^30.
struct XcdRemap {
  unsigned gx, gy;  // grid x, y (the logical grid is gx * gy * gz blocks, total = q * 8 + r)
  unsigned q, r;    // total >> 3, total & 7
  unsigned mx, sx;  // magic and shift of the division by gx
  unsigned my, sy;  // ... by gy (3-D grids; 2^31, 0 otherwise)
};
__host__ __device__ inline bool xcd_magic(unsigned d, unsigned long long total, unsigned* m, unsigned* s) {
  if (d == 0 || total == 0 || total > (1ull << 30)) return false;
  for (unsigned sh = 0; sh < 32; sh++) {
    const unsigned long long p = 1ull << (31 + sh), mm = (p + d - 1) / d;
    if (mm >> 32) break;
    if ((2 * total - 1) * (mm * d - p) < p) {
      *m = (unsigned)mm;
      *s = sh;
      return true;
    }
  }
  return false;
}
__host__ __device__ inline bool make_xcd_remap(unsigned gx, unsigned gy, unsigned gz, XcdRemap* R) {
  const unsigned long long total = (unsigned long long)gx * gy * gz;
  if (!xcd_magic(gx, total, &R->mx, &R->sx) || !xcd_magic(gy, total, &R->my, &R->sy)) return false;
  R->gx = gx;
  R->gy = gy;
  R->q = (unsigned)(total >> 3);
  R->r = (unsigned)(total & 7);
  return true;
}
__device__ __forceinline__ unsigned xcd_div(unsigned l, unsigned m, unsigned s) { return __umulhi(2u * l + 1u, m) >> s; }
__device__ __forceinline__ unsigned xcd_block(unsigned hw, const XcdRemap& R) {
  const unsigned x = hw & 7;
  return x * R.q + min(x, R.r) + (hw >> 3);
}
__device__ __forceinline__ int2 xcd_block2(const XcdRemap& R) {
  const unsigned l = xcd_block(blockIdx.x + R.gx * blockIdx.y, R);
  const unsigned q = xcd_div(l, R.mx, R.sx);
  return make_int2((int)(l - q * R.gx), (int)q);
}
__device__ __forceinline__ int3 xcd_block3(const XcdRemap& R) {
  const unsigned l = xcd_block(blockIdx.x + R.gx * (blockIdx.y + R.gy * blockIdx.z), R);
  const unsigned q = xcd_div(l, R.mx, R.sx), z = xcd_div(q, R.my, R.sy);
  return make_int3((int)(l - q * R.gx), (int)(q - z * R.gy), (int)z);
}

__device__ __forceinline__ int round_even(float v) { return (int)__builtin_rintf(v); }

// fastAtan2 (OpenCV 3.2 core): degrees in [0,360).
__device__ __forceinline__ float fast_atan2(float y, float x) {
  const float p1 = 0.9997878412794807f * (float)(180 / 3.14159265358979323846);
  const float p3 = -0.3258083974640975f * (float)(180 / 3.14159265358979323846);
  const float p5 = 0.1555786518463281f * (float)(180 / 3.14159265358979323846);
  const float p7 = -0.04432655554792128f * (float)(180 / 3.14159265358979323846);
  const float eps = (float)2.2204460492503131e-16;  // (float)DBL_EPSILON
  float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
  float a, c, c2;
  if (ax >= ay) {
    c = ay / (ax + eps);
    c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    c = ax / (ay + eps);
    c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

// Deterministic float sin/cos: double-precision Cody-Waite reduction + Taylor
// polynomials, rounded once to float (same operation sequence as the CPU
// restatement).  The 23 constants sit in a constant-memory
// table: a few wide scalar loads instead of two s_mov_b32 per double on the
// (scalar-issue-bound) describe path.  x - c is x + (-c) exactly, so the table
// holds the polynomial coefficients with their signs.
// K: the 23 constants in this order (extract.hip's c_sincos).
__device__ __forceinline__ void sincos_det(float xf, const double* __restrict__ K, float* s_out, float* c_out) {
  const double x = (double)xf;
  double kd = __builtin_rint(x * K[0]);
  int q = (int)kd;
  double r = (x - kd * K[1]) - kd * K[2];
  double r2 = r * r;
  double ps = K[3];
#pragma unroll
  for (int i = 4; i < 13; i++) ps = ps * r2 + K[i];
  double sr = r + r * (r2 * ps);
  double pc = K[13];
#pragma unroll
  for (int i = 14; i < 23; i++) pc = pc * r2 + K[i];
  double cr = 1.0 + r2 * pc;
  double s, c;
  switch (q & 3) {
    case 0: s = sr; c = cr; break;
    case 1: s = cr; c = -sr; break;
    case 2: s = -sr; c = -cr; break;
    default: s = -cr; c = sr; break;
  }
  *s_out = (float)s;
  *c_out = (float)c;
}

// Double sin/cos by Cody-Waite reduction + Taylor polynomials: basic IEEE operations only, so the
// CPU restatements reproduce it bit for bit (SE3Quat::exp in poseopt.hip, cv::Rodrigues in sim3.hip).
__host__ __device__ __forceinline__ void sincos_d(double x, double* s_out, double* c_out) {
  const double kInvPio2 = 6.36619772367581382433e-01;
  const double kPio2Hi = 1.57079632673412561417e+00;
  const double kPio2Lo = 6.07710050650619224932e-11;
  const double kd = __builtin_rint(x * kInvPio2);
  const int q = (int)kd;
  const double r = (x - kd * kPio2Hi) - kd * kPio2Lo;
  const double r2 = r * r;
  double ps = 1.0 / 51090942171709440000.0;
  ps = ps * r2 - 1.0 / 121645100408832000.0;
  ps = ps * r2 + 1.0 / 355687428096000.0;
  ps = ps * r2 - 1.0 / 1307674368000.0;
  ps = ps * r2 + 1.0 / 6227020800.0;
  ps = ps * r2 - 1.0 / 39916800.0;
  ps = ps * r2 + 1.0 / 362880.0;
  ps = ps * r2 - 1.0 / 5040.0;
  ps = ps * r2 + 1.0 / 120.0;
  ps = ps * r2 - 1.0 / 6.0;
  const double sr = r + r * (r2 * ps);
  double pc = 1.0 / 2432902008176640000.0;
  pc = pc * r2 - 1.0 / 6402373705728000.0;
  pc = pc * r2 + 1.0 / 20922789888000.0;
  pc = pc * r2 - 1.0 / 87178291200.0;
  pc = pc * r2 + 1.0 / 479001600.0;
  pc = pc * r2 - 1.0 / 3628800.0;
  pc = pc * r2 + 1.0 / 40320.0;
  pc = pc * r2 - 1.0 / 720.0;
  pc = pc * r2 + 1.0 / 24.0;
  pc = pc * r2 - 0.5;
  const double cr = 1.0 + r2 * pc;
  double s, c;
  switch (q & 3) {
    case 0: s = sr; c = cr; break;
    case 1: s = cr; c = -sr; break;
    case 2: s = -sr; c = -cr; break;
    default: s = -cr; c = sr; break;
  }
  *s_out = s;
  *c_out = c;
}

// Double e^x from basic IEEE operations only (g2o::Sim3's std::exp(sigma) in optsim3.hip), the same
// sequence in the tests' Python twin: k = rint(x / ln 2), r = (x - k ln2_hi) - k ln2_lo (Cody-Waite,
// |r| < 0.3466), e^r = 1 + (r + r^2 p(r)) with p the Taylor series of (e^r - 1 - r) / r^2 to r^11 by
// Horner (truncation below 0.06 units of 2^-53), times 2^k built from its exponent bits (exact; k is
// clamped to the normal exponents, domain |x| <= 708).  exp_det(0) is exactly 1.  Against the true
// exponential the result is within 2.5 * 2^-53 relative for |x| <= 2 (derived term by term in
// tests/optsim3_literal.py).
__host__ __device__ inline double exp_det(double x) {
  if (x != x) return x;
  double kd = __builtin_rint(x * 1.44269504088896338700e+00);
  kd = kd > 1023.0 ? 1023.0 : kd;
  kd = kd < -1022.0 ? -1022.0 : kd;
  const double r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;
  double p = 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  const double e = 1.0 + (r + (r * r) * p);
  const long long bits = ((long long)kd + 1023) << 52;
  double scale;
  __builtin_memcpy(&scale, &bits, sizeof(scale));
  return e * scale;
}

// Double atan2 from basic IEEE operations only (+ - * / rint, compares), the same sequence on the
// host, the device and in the tests' Python twin; std::atan2's special values (signed zeros, axes,
// infinities, NaN).  t = min(|y|,|x|) / max(|y|,|x|) in [0,1]; atan t = atan c + atan((t-c)/(1+tc))
// with c the nearest multiple of 1/4, |(t-c)/(1+tc)| <= 1/8, odd series to r^23 (truncation
// below 1e-23); then the octant, half-plane and sign folds with two-word pi/2 and pi.
__host__ __device__ inline double atan2_det(double y, double x) {
  if (y != y || x != x) return y + x;
  const bool ny = __builtin_signbit(y), nx = __builtin_signbit(x);
  const double ay = ny ? -y : y, ax = nx ? -x : x;
  const bool sw = ay > ax;
  const double hi = sw ? ay : ax, lo = sw ? ax : ay;
  double t;
  if (hi == 0.0)
    t = 0.0;
  else if (lo == hi)  // also inf / inf
    t = 1.0;
  else
    t = lo / hi;
  const double k = __builtin_rint(t * 4.0);
  const double c = k * 0.25;
  const double base = k == 0.0   ? 0.0
                      : k == 1.0 ? 2.44978663126864143e-01
                      : k == 2.0 ? 4.63647609000806094e-01
                      : k == 3.0 ? 6.43501108793284371e-01
                                 : 7.85398163397448279e-01;
  const double r = (t - c) / (1.0 + t * c);
  const double r2 = r * r;
  double p = 1.0 / 23.0;
  p = p * r2 - 1.0 / 21.0;
  p = p * r2 + 1.0 / 19.0;
  p = p * r2 - 1.0 / 17.0;
  p = p * r2 + 1.0 / 15.0;
  p = p * r2 - 1.0 / 13.0;
  p = p * r2 + 1.0 / 11.0;
  p = p * r2 - 1.0 / 9.0;
  p = p * r2 + 1.0 / 7.0;
  p = p * r2 - 1.0 / 5.0;
  p = p * r2 + 1.0 / 3.0;
  double a = base + (r - r * (r2 * p));
  if (sw) a = (1.57079632679489656e+00 - a) + 6.12323399573676604e-17;
  if (nx) a = (3.14159265358979312e+00 - a) + 1.22464679914735321e-16;
  return ny ? -a : a;
}

// Float acos (Initializer::CheckRT's acos(float)) from basic IEEE operations only: the double
// acos x = atan2(sqrt((1 - x)(1 + x)), x) through atan2_det, rounded once to float; the same sequence
// on the host, the device and in the tests' Python twin.  1 - x and 1 + x are exact in double for
// every float |x| >= 2^-29; |x| > 1 gives NaN (the square root of a negative), -0 counts as +0.
__host__ __device__ inline float acosf_det(float x) {
  if (x == 0.f) x = 0.f;
  const double xd = (double)x;
  return (float)atan2_det(__builtin_sqrt((1.0 - xd) * (1.0 + xd)), xd);
}

// Double natural logarithm from basic IEEE operations only (g2o::Sim3::log's std::log(s) in
// essgraph.hip), the same sequence in the tests' Python twin.  Domain: positive normal doubles (a zero,
// negative, subnormal, infinite or NaN argument gives NaN: a Sim3 scale is none of these).
// x = m 2^k from the exponent bits with m in (sqrt(1/2), sqrt 2] (exact); f = m - 1 (exact, Sterbenz);
// s = f / (2 + f), |s| <= 0.1716; ln m = 2 atanh s = 2s + s (z P(z)), z = s*s, P the series
// 2/3 + 2z/5 + ... + 2 z^10 / 23 by Horner (truncation below 2e-20 relative); the result is
// k ln2_hi + (ln m + k ln2_lo), k ln2_hi exact (ln2_hi has 21 trailing zero bits).  log_det(1) is
// exactly 0: k = 0, f = 0, s = 0 and every term is 0.  Against the true logarithm the result is
// within 6 * 2^-53 relative (derived term by term in tests/essgraph_literal.py).
__host__ __device__ inline double log_det(double x) {
  if (!(x >= 2.2250738585072014e-308 && x <= 1.7976931348623157e308)) return __builtin_nan("");
  long long bits;
  __builtin_memcpy(&bits, &x, sizeof(bits));
  long long k = ((bits >> 52) & 0x7ff) - 1023;
  long long mb = (bits & 0x000fffffffffffffLL) | 0x3ff0000000000000LL;  // m in [1, 2)
  double m;
  __builtin_memcpy(&m, &mb, sizeof(m));
  if (m > 1.41421356237309514547e+00) {
    m = m * 0.5;
    k = k + 1;
  }
  const double kd = (double)k;
  const double f = m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s;
  double p = 2.0 / 23.0;
  p = p * z + 2.0 / 21.0;
  p = p * z + 2.0 / 19.0;
  p = p * z + 2.0 / 17.0;
  p = p * z + 2.0 / 15.0;
  p = p * z + 2.0 / 13.0;
  p = p * z + 2.0 / 11.0;
  p = p * z + 2.0 / 9.0;
  p = p * z + 2.0 / 7.0;
  p = p * z + 2.0 / 5.0;
  p = p * z + 2.0 / 3.0;
  const double lm = (s + s) + s * (z * p);
  return kd * 6.93147180369123816490e-01 + (lm + kd * 1.90821492927058770002e-10);
}

// Double acos (g2o::Sim3::log's acos(d)) from basic IEEE operations only:
// acos x = atan2(sqrt((1 - x)(1 + x)), x) through atan2_det, acosf_det's sequence without the final
// rounding to float; |x| > 1 gives NaN (the square root of a negative), -0 counts as +0.  Within
// 20 * 2^-53 relative of the true arc cosine on [-1, 1) (derived in tests/essgraph_literal.py);
// acos_det(1) is exactly 0.
__host__ __device__ inline double acos_det(double x) {
  if (x == 0.0) x = 0.0;
  return atan2_det(__builtin_sqrt((1.0 - x) * (1.0 + x)), x);
}

// Hamming distance of two 256-bit descriptors held as 4 x u64.
__device__ __forceinline__ int hamming256(const uint64_t a[4], const uint64_t b[4]) {
  return __popcll(a[0] ^ b[0]) + __popcll(a[1] ^ b[1]) + __popcll(a[2] ^ b[2]) + __popcll(a[3] ^ b[3]);
}

// Wave (64-lane) reductions.
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    uint32_t w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

// Ordered compaction of one chunk of kBS items (one per thread, every thread of the block calls):
// thread tid's kept item goes to slot base + (the kept items of lower threads); put(slot) stores it.
// base advances by the chunk's kept count.  A slot never lies above the item's own position in the
// list, so a caller may compact in place.  scan: kBS / 64 ints of LDS.
template <int kBS, class Put>
__device__ __forceinline__ void compact_chunk(bool keep, int* scan, int& base, Put put) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t m = __ballot(keep);
  const int pre = __popcll(m & ((1ull << lane) - 1));
  if (lane == 0) scan[wid] = __popcll(m);
  __syncthreads();  // (every item of this chunk has been read by now)
  int off = base;
  for (int w = 0; w < wid; w++) off += scan[w];
  if (keep) put(off + pre);
  int tot = 0;
  for (int w = 0; w < kBS / 64; w++) tot += scan[w];
  base += tot;
  __syncthreads();
}

}  // namespace orbx

// ba_math.h -- LocalBundleAdjustment (localba.hip): quaternion / SE3 numerics, 3x3 inverse, and the
// fixed-order reductions (wave butterflies, block sums, the two sums over block partials:
// fixed_sum_wave's lane-strided tree and index_order_sum_wave's index order).
#pragma once
#include "ba_types.h"

namespace orbx {

// ------------------------------------------------------------ SE3 numerics
struct Quat {
  double x, y, z, w;
};

__host__ __device__ inline Quat qmul(const Quat& a, const Quat& b) {
  Quat r;
  r.w = a.w * b.w - (a.x * b.x + a.y * b.y + a.z * b.z);
  r.x = a.w * b.x + b.w * a.x + (a.y * b.z - a.z * b.y);
  r.y = a.w * b.y + b.w * a.y + (a.z * b.x - a.x * b.z);
  r.z = a.w * b.z + b.w * a.z + (a.x * b.y - a.y * b.x);
  return r;
}

// Eigen Quaternion * Vector3 (_transformVector)
__host__ __device__ inline void qrot(const Quat& q, const double v[3], double out[3]) {
  double uv[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
  uv[0] += uv[0];
  uv[1] += uv[1];
  uv[2] += uv[2];
  const double c[3] = {q.y * uv[2] - q.z * uv[1], q.z * uv[0] - q.x * uv[2], q.x * uv[1] - q.y * uv[0]};
  for (int i = 0; i < 3; i++) out[i] = v[i] + q.w * uv[i] + c[i];
}

__host__ __device__ inline void qmat(const Quat& q, double R[9]) {
  const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

__host__ __device__ inline Quat mat2q(const double m[9]) {
  Quat q;
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q.w = 0.5 * t;
    t = 0.5 / t;
    q.x = (m[7] - m[5]) * t;
    q.y = (m[2] - m[6]) * t;
    q.z = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[3 * i + i]) i = 2;
    // the three cases spelled out on named entries: no array indexed at run time (which put the
    // matrix in scratch memory); same arithmetic as c[i], c[j], c[k] with (i, j, k) cyclic
    if (i == 0) {  // (0, 1, 2)
      t = sqrt(m[0] - m[4] - m[8] + 1.0);
      const double ci = 0.5 * t;
      t = 0.5 / t;
      q.w = (m[7] - m[5]) * t;
      q.x = ci;
      q.y = (m[3] + m[1]) * t;
      q.z = (m[6] + m[2]) * t;
    } else if (i == 1) {  // (1, 2, 0)
      t = sqrt(m[4] - m[8] - m[0] + 1.0);
      const double ci = 0.5 * t;
      t = 0.5 / t;
      q.w = (m[2] - m[6]) * t;
      q.y = ci;
      q.z = (m[7] + m[5]) * t;
      q.x = (m[1] + m[3]) * t;
    } else {  // (2, 0, 1)
      t = sqrt(m[8] - m[0] - m[4] + 1.0);
      const double ci = 0.5 * t;
      t = 0.5 / t;
      q.w = (m[3] - m[1]) * t;
      q.z = ci;
      q.x = (m[2] + m[6]) * t;
      q.y = (m[5] + m[7]) * t;
    }
  }
  return q;
}

__host__ __device__ inline void qnormalize(Quat& q) {
  if (q.w < 0) {
    q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w;
  }
  const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  q.x /= n; q.y /= n; q.z /= n; q.w /= n;
}

struct SE3d {
  Quat q;
  double t[3];
};

__device__ inline SE3d se3_exp(const double u[6]) {
  const double w[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]};
  const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double O[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double O2[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) O2[3 * r + c] = O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c] + O[3 * r + 2] * O[6 + c];
  double R[9], V[9];
  if (theta < 0.00001) {
    for (int i = 0; i < 9; i++) R[i] = ((i % 4) == 0 ? 1.0 : 0.0) + O[i] + O2[i];
    for (int i = 0; i < 9; i++) V[i] = R[i];
  } else {
    const double s = sin(theta), c = cos(theta);
    const double a = s / theta, b = (1 - c) / (theta * theta), d = (theta - s) / pow(theta, 3);
    for (int i = 0; i < 9; i++) {
      const double I = (i % 4) == 0 ? 1.0 : 0.0;
      R[i] = I + a * O[i] + b * O2[i];
      V[i] = I + b * O[i] + d * O2[i];
    }
  }
  SE3d T;
  T.q = mat2q(R);
  for (int r = 0; r < 3; r++) T.t[r] = V[3 * r] * up[0] + V[3 * r + 1] * up[1] + V[3 * r + 2] * up[2];
  qnormalize(T.q);
  return T;
}

__device__ inline void inv3(const double m[9], double out[9]) {
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  const double id = 1.0 / det;
  out[0] = c00 * id;
  out[1] = (m[2] * m[7] - m[1] * m[8]) * id;
  out[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  out[3] = c01 * id;
  out[4] = (m[0] * m[8] - m[2] * m[6]) * id;
  out[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  out[6] = c02 * id;
  out[7] = (m[1] * m[6] - m[0] * m[7]) * id;
  out[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// Cross-lane exchange with the partner lane for butterfly level O: xor 32 via
// ds_bpermute, xor 16 via ds_swizzle, and the in-row levels through DPP (no
// LDS traffic): row_mirror (i <-> 15-i), row_half_mirror (i <-> 7-i), quad
// perms.  Each is an involution whose partner differs in bit O of the lane.
template <int O>
__device__ inline int xlane_i(int x) {
  if constexpr (O == 32) return __shfl_xor(x, 32, 64);
  else if constexpr (O == 16) return __builtin_amdgcn_ds_swizzle(x, (0x10 << 10) | 0x1F);
  else if constexpr (O == 8) return __builtin_amdgcn_mov_dpp(x, 0x140, 0xF, 0xF, false);
  else if constexpr (O == 4) return __builtin_amdgcn_mov_dpp(x, 0x141, 0xF, 0xF, false);
  else if constexpr (O == 2) return __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, false);
  else return __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, false);
}
template <int O>
__device__ inline double xlane(double v) {
  const long long x = __double_as_longlong(v);
  const int lo = xlane_i<O>((int)x), hi = xlane_i<O>((int)(x >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// Butterfly sum of one double over the 64 lanes (every lane gets the total).
template <int O = 32>
__device__ inline double wave_sum(double v) {
  v += xlane<O>(v);
  if constexpr (O > 1) return wave_sum<O / 2>(v);
  else return v;
}

// Reduce-scatter of M per-lane values over the wave by recursive halving: at
// level O the lanes with bit O set keep the upper half and send the lower,
// so only M/2 values cross lanes per level (M-1 exchanges in all instead of
// 6M).  On exit w[0] of every lane is the wave total of value idx.
template <int M, int O>
__device__ inline void wave_reduce_scatter(double* w, int lane, int& idx) {
  if constexpr (O > 0) {
    const bool hi = (lane & O) != 0;
    if constexpr (M > 1) {
#pragma unroll
      for (int i = 0; i < M / 2; i++) {
        const double keep = hi ? w[M / 2 + i] : w[i];
        const double send = hi ? w[i] : w[M / 2 + i];
        w[i] = keep + xlane<O>(send);
      }
      if (hi) idx += M / 2;
      wave_reduce_scatter<M / 2, O / 2>(w, lane, idx);
    } else {
      w[0] += xlane<O>(w[0]);
      wave_reduce_scatter<1, O / 2>(w, lane, idx);
    }
  }
}

// Fixed-order block sum of one double per thread (blockDim LBS); every thread gets the result.
__device__ inline double block_sum1(double v, double* red /* LDS [LBS/64] */) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0;
#pragma unroll
  for (int w = 0; w < LBS / 64; w++) s += red[w];
  __syncthreads();
  return s;
}

// Block partial of a grid-wide sum: stored to out[blockIdx.x], no cross-block
// synchronisation on the device.  The partials are summed later in one of two
// fixed orders: index (block) order by the host after a readback and by
// index_order_sum_wave (the reported chi2, the host-controlled loop), or
// fixed_sum_wave's lane-strided tree (the device LM verdict's chi and scale).
__device__ inline void block_partial(double v, double* out, double* out2 = nullptr) {
  __shared__ double red[LBS / 64];
  const double bs = block_sum1(v, red);
  if (threadIdx.x == 0) {
    out[blockIdx.x] = bs;
    if (out2) out2[blockIdx.x] = bs;
  }
}

// Relaxed agent-scope store / load of a double: written through / read past the XCD's L2, so a
// value one block stores is seen by another block of the same launch (k_ba_errors_ctl's partials)
__device__ inline void st_agent(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline double ld_agent(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p),
                                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// Fixed-order block sum of NV per-thread partials over a kGB-thread block
// (shuffle tree per wave, then the waves' results summed in wave order by
// thread j < NV): deterministic for a fixed launch shape.  Returns the NV
// totals (in LDS, visible to the whole block).
template <int NV, int NW = kGW>
__device__ inline const double* block_sum_fixed(double (&v)[NV], double* red /* LDS [(NW+1)*NV] */) {
  static_assert(NV <= 64, "one value per lane after the reduce-scatter");
  constexpr int P = NV <= 1 ? 1 : NV <= 2 ? 2 : NV <= 4 ? 4 : NV <= 8 ? 8 : NV <= 16 ? 16 : NV <= 32 ? 32 : 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double w[P];
#pragma unroll
  for (int j = 0; j < P; j++) w[j] = j < NV ? v[j] : 0.0;
  int idx = 0;
  wave_reduce_scatter<P, 32>(w, lane, idx);
  if (idx < NV && (lane & ((64 / P) - 1)) == 0) red[wv * NV + idx] = w[0];
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) t += red[w * NV + threadIdx.x];
    red[NW * NV + threadIdx.x] = t;
  }
  __syncthreads();
  return red + NW * NV;
}

// Chunk s of S of the range [lo, hi): [lo + n*s/S, lo + n*(s+1)/S).
__device__ inline void chunk_range(int lo, int hi, int s, int S, int& a, int& b) {
  const long long n = hi - lo;
  a = lo + (int)(n * s / S);
  b = lo + (int)(n * (s + 1) / S);
}

// Sum of n block partials in a fixed order, by one wave: lane l adds p[l], p[l + 64], ... in index
// order (eight loads in flight per round), then a butterfly over the 64 lanes -- a lane-strided
// tree, NOT the index-order sum (index_order_sum_wave, the host readback): the two differ in their
// low bits.  Lane 0's value -- the one the LM verdict uses -- is the same bits on every run and in
// the batched driver.  (It replaced lane 0 adding all partials in sequence through LDS: a ~170-add
// FP64 chain per sum on the trial's critical path, and no barrier is needed now, so any wave of a
// block may call it.)
template <bool coh = false>  // coh: p is read with ld_agent (partials stored by this launch's other blocks)
__device__ inline double fixed_sum_wave(const double* p, int n) {
  const int lane = threadIdx.x & 63;
  double s = 0;
  for (int base = 0; base < n; base += 512) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {  // clamped, unpredicated loads: all eight in flight at once
      const int i = max(min(base + lane + 64 * u, n - 1), 0);
      v[u] = coh ? ld_agent(p + i) : p[i];
    }
#pragma unroll
    for (int u = 0; u < 8; u++) s += base + lane + 64 * u < n ? v[u] : 0.0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}
// The host readback's order (partials added in index order, lane 0; block = one wave): the batched
// driver's reported final chi, which must equal the single driver's host-side sum bit for bit.
__device__ inline double index_order_sum_wave(const double* p, int n) {
  __shared__ double buf[1024];
  double s = 0;
  for (int base = 0; base < n; base += 1024) {
    const int m = min(1024, n - base);
    for (int i = threadIdx.x; i < m; i += 64) buf[i] = p[base + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; i++) s += buf[i];
    __syncthreads();
  }
  return s;
}
// two fixed_sum_wave sums (the verdict's chi and LM scale); valid in lane 0 of every calling wave
template <bool coh = false>
__device__ inline void fixed_sum2_wave(const double* p, int n, const double* q, int m, double& sp, double& sq) {
  sp = fixed_sum_wave<coh>(p, n);
  sq = fixed_sum_wave<false>(q, m);
}

}  // namespace orbx

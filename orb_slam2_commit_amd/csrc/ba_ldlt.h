// ba_ldlt.h -- LocalBundleAdjustment (localba.hip): dense LDLT and solve of the reduced camera
// system.  Three single-workgroup kernels -- 16-wide blocked MFMA (k_ba_ldlt), column-step with 4x4
// register tiles (k_ba_ldlt_col), 8-wide panels over those tiles (k_ba_ldlt_pan) --, the tiled
// kernels over many workgroups for a global map's system (k_ba_ldlt_tiled_*), and the plan that
// picks by size (LdltPlan).
#pragma once
#include <map>
#include <mutex>
#include <utility>

#include "ba_math.h"

namespace orbx {

__device__ inline double readlane_d(double v, int l) {
  const long long x = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)x, l);
  const int hi = __builtin_amdgcn_readlane((int)(x >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int kLdltMaxNp = 1024;                // padded size limit (panel buffer Np x 17 doubles in LDS)
constexpr int kLdltLdsNp = 128;                 // largest padded size kept in LDS
inline int ldlt_np(int N) { return (N + 15) & ~15; }
inline size_t ldlt_smem_bytes(int N, bool lds) {
  const size_t Np = ldlt_np(N);
  return ((lds ? Np * (Np + 1) : 0) + Np * 17) * sizeof(double);
}

// Dense LDLT (no pivoting; fails on an exactly zero pivot like Eigen's
// SimplicialLDLT) of the N x N reduced camera system and the solve, blocked
// by 16-column panels.  The matrix is padded to Np = 16k with an identity
// block (decoupled, never a zero pivot).  Per panel:
//   1. wave 0 factors the 16 x 16 diagonal block in registers (lane r = row
//      r, column values broadcast with readlane);
//   2. each row below it solves its 16 panel entries against L11 (one
//      thread per row) and stores W = L D (in A) and L (in P);
//   3. the trailing lower triangle is updated A22 -= W21 L21^T with FP64
//      MFMA 16x16x4 tiles spread over the 16 waves.
// Then L = W / D in place, and the two triangular solves run on wave 0 with
// the vector in registers.  kLds: A in LDS (row stride Np+1), else in the
// global scratch D.Sw (row stride Np).  A template parameter, not a runtime
// select, so that LDS accesses are ds_* and not FLAT instructions.
#define LDLT_TS(idx)                                                  \
  do {                                                                \
    if (D.dbg && tid == 0 && (idx) < 64) D.dbg[idx] = __builtin_amdgcn_s_memtime(); \
  } while (0)
template <bool kLds>
__global__ __launch_bounds__(1024) void k_ba_ldlt(BaDev D, int stage_limit) {
  if (lm_skip(D)) return;
  extern __shared__ double sm[];
  __shared__ int fail;
  __shared__ double Dinv_p[16];
  const int N = 6 * D.nposes, Np = (N + 15) & ~15, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ld = kLds ? Np + 1 : Np;
  double* A = kLds ? sm : D.Sw;
  double* P = sm + (kLds ? (size_t)Np * ld : 0);  // Np x 16 (stride 17): L of the current panel
  for (int i0 = 0; i0 < Np * Np; i0 += 4 * 1024) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int idx = i0 + u * 1024 + tid, r = idx / Np, c = idx - r * Np;
      v[u] = (r < N && c < N) ? D.S[(size_t)r * N + c] : (r == c ? 1.0 : 0.0);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int idx = i0 + u * 1024 + tid, r = idx / Np, c = idx - r * Np;
      if (idx < Np * Np) A[(size_t)r * ld + c] = v[u];
    }
  }
  if (tid == 0) fail = 0;
  __syncthreads();
  LDLT_TS(0);
  if (stage_limit == 1) return;
  for (int j0 = 0; j0 < Np; j0 += 16) {
    if (wv == 0) {
      const int r = lane & 15;
      double row[16];
#pragma unroll
      for (int c = 0; c < 16; c++) row[c] = A[(size_t)(j0 + r) * ld + j0 + c];
      bool bad = false;  // no early exit: the loops must unroll fully (constant register indices)
#pragma unroll
      for (int c = 0; c < 16; c++) {
        const double d = readlane_d(row[c], c);
        bad |= d == 0.0;
        const double invd = 1.0 / d;
#pragma unroll
        for (int k = c + 1; k < 16; k++) {
          const double lk = readlane_d(row[c], k) * invd;  // L[k][c]
          if (r >= k) row[k] -= row[c] * lk;
        }
      }
      if (bad) {
        if (lane == 0) fail = 1;
      } else if (lane < 16) {
        const double dr = row[r < 16 ? r : 0];
        double dd[16];
#pragma unroll
        for (int c = 0; c < 16; c++) dd[c] = readlane_d(row[c], c);
#pragma unroll
        for (int c = 0; c < 16; c++) {
          if (c <= r) A[(size_t)(j0 + r) * ld + j0 + c] = row[c];
          if (c < r) P[(j0 + r) * 17 + c] = row[c] / dd[c];
        }
        Dinv_p[r] = 1.0 / dr;
      }
    }
    __syncthreads();
    LDLT_TS(1 + 3 * (j0 >> 4));
    if (fail) {
      if (tid == 0) D.scal[2] = 0.0;
      return;
    }
    const int nrows = Np - j0 - 16;
    for (int t = tid; t < nrows; t += 1024) {
      const int i = j0 + 16 + t;
      double w[16];
#pragma unroll
      for (int c = 0; c < 16; c++) w[c] = A[(size_t)i * ld + j0 + c];
#pragma unroll
      for (int c = 1; c < 16; c++)
#pragma unroll
        for (int m = 0; m < c; m++) w[c] -= w[m] * P[(j0 + c) * 17 + m];
#pragma unroll
      for (int c = 0; c < 16; c++) {
        A[(size_t)i * ld + j0 + c] = w[c];
        P[i * 17 + c] = w[c] * Dinv_p[c];
      }
    }
    __syncthreads();
    LDLT_TS(2 + 3 * (j0 >> 4));
    const int m = nrows >> 4, T = m * (m + 1) / 2;
    for (int t = wv; t < T; t += 16) {
      int ti = (int)((sqrtf(8.f * t + 1.f) - 1.f) * 0.5f);
      while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
      while (ti * (ti + 1) / 2 > t) ti--;
      const int tk = t - ti * (ti + 1) / 2;
      const int R0 = j0 + 16 + 16 * ti, C0 = j0 + 16 + 16 * tk;
      double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < 4; kk++) {
        const double av = A[(size_t)(R0 + (lane & 15)) * ld + j0 + 4 * kk + (lane >> 4)];  // W[row][k]
        const double bv = P[(C0 + (lane & 15)) * 17 + 4 * kk + (lane >> 4)];              // L[col][k]
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
      }
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const size_t o = (size_t)(R0 + (lane >> 4) + 4 * rr) * ld + C0 + (lane & 15);
        A[o] -= acc[rr];
      }
    }
    __syncthreads();
    LDLT_TS(3 + 3 * (j0 >> 4));
  }
  if (stage_limit == 2) return;
  for (int i = 1 + (tid >> 5); i < Np; i += 32)
    for (int k = tid & 31; k < i; k += 32) A[(size_t)i * ld + k] /= A[(size_t)k * ld + k];
  __syncthreads();
  LDLT_TS(60);
  if (stage_limit == 3) return;
  // blocked triangular solves with the vector in LDS (the panel buffer P is
  // free now): per 16-row panel wave 0 solves the small triangle in registers
  // (readlane broadcasts), then every thread updates the remaining rows
  double* yv = P;
  for (int i = tid; i < Np; i += 1024) yv[i] = i < N ? D.bs[i] : 0.0;
  __syncthreads();
  for (int j0 = 0; j0 < Np; j0 += 16) {  // L z = b (unit lower)
    if (wv == 0) {
      const int r = lane & 15;
      double Lr[16];
#pragma unroll
      for (int c = 0; c < 16; c++) Lr[c] = A[(size_t)(j0 + r) * ld + j0 + c];
      double val = yv[j0 + r];
#pragma unroll
      for (int c = 0; c < 16; c++) {
        const double zc = readlane_d(val, c);
        if (r > c) val -= Lr[c] * zc;
      }
      if (lane < 16) yv[j0 + r] = val;
    }
    __syncthreads();
    for (int i = j0 + 16 + tid; i < Np; i += 1024) {
      double sacc = yv[i];
#pragma unroll
      for (int c = 0; c < 16; c++) sacc -= A[(size_t)i * ld + j0 + c] * yv[j0 + c];
      yv[i] = sacc;
    }
    __syncthreads();
  }
  for (int i = tid; i < Np; i += 1024) yv[i] /= A[(size_t)i * ld + i];
  __syncthreads();
  for (int j0 = Np - 16; j0 >= 0; j0 -= 16) {  // L^T x = z
    if (wv == 0) {
      const int r = lane & 15;
      double Lc[16];
#pragma unroll
      for (int c = 0; c < 16; c++) Lc[c] = A[(size_t)(j0 + c) * ld + j0 + r];
      double val = yv[j0 + r];
#pragma unroll
      for (int c = 15; c >= 0; c--) {
        const double xc = readlane_d(val, c);
        if (r < c) val -= Lc[c] * xc;
      }
      if (lane < 16) yv[j0 + r] = val;
    }
    __syncthreads();
    for (int i = tid; i < j0; i += 1024) {
      double sacc = yv[i];
#pragma unroll
      for (int c = 0; c < 16; c++) sacc -= A[(size_t)(j0 + c) * ld + i] * yv[j0 + c];
      yv[i] = sacc;
    }
    __syncthreads();
  }
  for (int i = tid; i < N; i += 1024) D.xp[i] = yv[i];
  if (tid == 0) D.scal[2] = 1.0;
  LDLT_TS(61);
}

// ---- reduced camera system, small N: column-step LDLT with 4x4 tiles ----
// Right-looking LDL^T of the augmented [S b; b^T .] with one barrier per
// pivot (~780 cycles per pivot on gfx950, latency-bound: LDS round trip +
// reciprocal + barrier; 60 us at N = 120 vs 71 us for the 16-wide blocked
// kernel, whose in-wave panel factorisation is readlane/division bound).  Each thread owns TPT 4x4 tiles of the lower triangle in registers
// (rows up to N, row N = rhs, padded to a multiple of 4).  At pivot j a tile
// reads 4 + 4 entries of column j from LDS (two ds_read_b128 each) and does
// 16 FMAs -- a quarter of the LDS traffic of one element per thread, which
// is what bounds this loop.  After pivot j's update the owners of column
// j+1 publish it (and 1/d_{j+1}) to LDS; nothing else is read from LDS.  The
// augmented row ends as z = L^-1 b (columns are unscaled: entry (i,j) =
// L_ij d_j), so the forward solve is free; wave 0 then applies D^-1 and the
// backward L^T solve, prefetching column entries eight pivots at a time.  A
// zero pivot fails the solve (scal[2] = 0) like the blocked kernel.
//
// LDS column j holds rows (j & ~3) .. Np4-1 at Lc[cbase(j) + i], 32-byte
// aligned for every 4-row group.
__host__ __device__ inline int ldlt_np4(int N) { return (N + 1 + 3) & ~3; }
__host__ __device__ inline int ldlt_cstart(int j, int N) {  // sum_{c<j} (Np4 - (c & ~3))
  const int q = j >> 2, r = j & 3;
  return j * ldlt_np4(N) - (8 * q * (q - 1) + 4 * q * r);
}
__host__ __device__ inline int ldlt_cbase(int j, int N) { return ldlt_cstart(j, N) - (j & ~3); }
inline int ldlt_col_tiles(int N) {
  const int Tr = ldlt_np4(N) / 4, Tc = (N + 3) / 4;
  return Tc * Tr - Tc * (Tc - 1) / 2;
}
inline size_t ldlt_col_smem(int N) { return (size_t)(ldlt_cstart(N, N) + N + 1) * sizeof(double); }
constexpr size_t kLdltColMaxSmem = 160 * 1024 - 256;
constexpr int kLdltColNT = 1024;        // threads of k_ba_ldlt_col
constexpr int kLdltColMaxTiles = 2048;  // at most two register tiles per thread
inline bool ldlt_col_fits(int N) {
  return ldlt_col_smem(N) <= kLdltColMaxSmem && ldlt_col_tiles(N) <= kLdltColMaxTiles;
}

typedef double double2_t __attribute__((ext_vector_type(2)));

// 1/d by v_rcp_f64 + two Newton steps (full double accuracy, a third of the
// latency of the IEEE division sequence -- it sits on the per-pivot path).
__device__ inline double rcp_nr(double d) {
  double r = __builtin_amdgcn_rcp(d);
  double e = fma(-d, r, 1.0);
  r = fma(r, e, r);
  e = fma(-d, r, 1.0);
  return fma(r, e, r);
}

// Pivot j = 4m + U of k_ba_ldlt_col: rank-1 update of the active tiles from
// column j, then the owners of column j+1 publish it and 1/d_{j+1}.  The updates (and the
// back solve's) are explicit FMAs: one FP64 op per link of the chain instead of a multiply and
// a subtract (60 -> 55 us at N = 120).  The solve is tested against numpy (1e-10) and through the
// LM decisions against the oracle; no other path shares its rounding.
template <int TPT, int U>
__device__ __forceinline__ void ldlt_col_step(double* Lc, double* rinv, double (&a)[TPT][4][4], const int (&ti)[TPT],
                                              const int (&tk)[TPT], int m, int N, int& fail) {
  const int j = 4 * m + U;
  if (j >= N) return;  // uniform
  const double* cj = Lc + ldlt_cbase(j, N);
  const double invd = rinv[j];
#pragma unroll
  for (int t = 0; t < TPT; t++) {
    if (tk[t] >= m && !(tk[t] == m && U == 3)) {  // some column of the tile is > j
      const double2_t* pr = reinterpret_cast<const double2_t*>(cj + 4 * ti[t]);
      const double2_t* pk = reinterpret_cast<const double2_t*>(cj + 4 * tk[t]);
      const double2_t r0 = pr[0], r1 = pr[1], k0 = pk[0], k1 = pk[1];
      const double cr[4] = {r0.x, r0.y, r1.x, r1.y}, ckv[4] = {k0.x, k0.y, k1.x, k1.y};
      double ck[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const bool live = (tk[t] > m || q > U) && 4 * tk[t] + q < N;
        ck[q] = live ? ckv[q] * invd : 0.0;  // select: junk never propagates
      }
#pragma unroll
      for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) a[t][p][q] = __builtin_fma(-cr[p], ck[q], a[t][p][q]);  // one op per link
    }
  }
  constexpr int Q = (U + 1) & 3;  // column j+1 within its tile
  const int mn = U == 3 ? m + 1 : m;
  if (j + 1 < N) {
#pragma unroll
    for (int t = 0; t < TPT; t++) {
      if (tk[t] == mn) {
        double2_t* dst = reinterpret_cast<double2_t*>(Lc + ldlt_cbase(j + 1, N) + 4 * ti[t]);
        dst[0] = double2_t{a[t][0][Q], a[t][1][Q]};
        dst[1] = double2_t{a[t][2][Q], a[t][3][Q]};
        if (ti[t] == tk[t]) {
          const double dn = a[t][Q][Q];
          rinv[j + 1] = rcp_nr(dn);
          if (dn == 0.0) fail = 1;
        }
      }
    }
  }
  __syncthreads();
}

template <int TPT, int NT>
__device__ __forceinline__ void k_ba_ldlt_col_body(const BaDev& D) {
  if (lm_skip(D) || D.ldlt_pan) return;
  extern __shared__ __attribute__((aligned(16))) double Lc[];
  __shared__ int fail;
  const int N = 6 * D.nposes, tid = threadIdx.x;
  const int Np4 = ldlt_np4(N), Tr = Np4 / 4, Tc = (N + 3) / 4;
  const int ntiles = Tc * Tr - Tc * (Tc - 1) / 2;
  double* rinv = Lc + ldlt_cstart(N, N);
  double a[TPT][4][4];
  int ti[TPT], tk[TPT];
  if (tid == 0) fail = 0;
#pragma unroll
  for (int t = 0; t < TPT; t++) {
    int x = tid + NT * t, k = 0;
    ti[t] = 0;
    tk[t] = -1;  // inactive
    if (x < ntiles) {
      while (x >= Tr - k) {  // column-major tile order
        x -= Tr - k;
        k++;
      }
      tk[t] = k;
      ti[t] = k + x;
    }
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int i = 4 * ti[t] + p, kk = 4 * tk[t] + q;
        double v = 0.0;
        if (tk[t] >= 0 && kk < N) v = i < N ? D.S[(size_t)i * N + kk] : (i == N ? D.bs[kk] : 0.0);
        a[t][p][q] = v;
      }
    if (tk[t] == 0) {
#pragma unroll
      for (int p = 0; p < 4; p++) Lc[ldlt_cbase(0, N) + 4 * ti[t] + p] = a[t][p][0];
      if (ti[t] == 0) {
        rinv[0] = rcp_nr(a[t][0][0]);
        if (a[t][0][0] == 0.0) fail = 1;
      }
    }
  }
  __syncthreads();
  for (int m = 0; 4 * m < N; m++) {  // pivots j = 4m + U, U unrolled so tile columns index statically
    ldlt_col_step<TPT, 0>(Lc, rinv, a, ti, tk, m, N, fail);
    ldlt_col_step<TPT, 1>(Lc, rinv, a, ti, tk, m, N, fail);
    ldlt_col_step<TPT, 2>(Lc, rinv, a, ti, tk, m, N, fail);
    ldlt_col_step<TPT, 3>(Lc, rinv, a, ti, tk, m, N, fail);
  }
  if (fail) {
    if (tid == 0) D.scal[2] = 0.0;
    return;
  }
  if (tid >= 64) return;
  // y = D^-1 z; L^T x = y (x_k final at step k, rows i < k updated)
  const int lane = tid;
  double y[4], invd[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int i = lane + 64 * r;
    invd[r] = 0.0;
    y[r] = 0.0;
    if (i < N) {
      invd[r] = rinv[i];
      y[r] = Lc[ldlt_cbase(i, N) + N] * invd[r];
    }
  }
  int cb[4];  // column i's base; rows >= N clamp to a valid column (their Lv is zeroed)
#pragma unroll
  for (int r = 0; r < 4; r++) cb[r] = ldlt_cbase(min(lane + 64 * r, N - 1), N);
  for (int kb = N - 1; kb >= 0; kb -= 8) {
    double Lv[8][4];
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll
      for (int r = 0; r < 4; r++) {  // branchless: all 32 LDS reads issue together
        const int i = lane + 64 * r, k = kb - u;
        const double v = Lc[cb[r] + (i < k ? k : min(i, N - 1))];  // always a finite L entry
        Lv[u][r] = v * (i < k ? invd[r] : 0.0);  // L[k][i]; a multiply, so the load is unconditional
      }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int k = kb - u;
      if (k >= 0) {
        const int rk = k >> 6;
        const double yk = rk == 0 ? y[0] : rk == 1 ? y[1] : rk == 2 ? y[2] : y[3];
        const double xk = readlane_d(yk, k & 63);
#pragma unroll
        for (int r = 0; r < 4; r++) y[r] = __builtin_fma(-Lv[u][r], xk, y[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++)
    if (lane + 64 * r < N) D.xp[lane + 64 * r] = y[r];
  if (lane == 0) D.scal[2] = 1.0;
}
template <int TPT, int NT>
__global__ __launch_bounds__(NT) void k_ba_ldlt_col(BaDev D) { k_ba_ldlt_col_body<TPT, NT>(D); }
template <int TPT, int NT>
__global__ __launch_bounds__(NT) void k_ba_ldlt_col_many(const BaDev* __restrict__ Ds) {
  k_ba_ldlt_col_body<TPT, NT>(Ds[blockIdx.z]);
}

// ---- reduced camera system: 8-wide panels over the column-step kernel's register tiles ----
// The column-step kernel pays one barrier and one LDS round trip per pivot; its per-pivot chain
// (publish column j+1 and 1/d, barrier, read, scale, update) is what bounds it.  Here the pivots
// go eight at a time.  Per panel M (columns c0 = 8M .. c0+7, tile columns 2M, 2M+1):
//   B  one thread per row i = c0 .. N (the augmented row b^T included) reads the panel's 8x8
//      diagonal block and its own row from LDS, factors the diagonal block in registers (every
//      such thread the same way: no cross-lane broadcast on the pivot chain) and solves its row:
//      L_i (scaled) and V_i = L_i D (unscaled) to LDS, L_i also into the packed factor;
//   C  every register tile right of the next panel takes A -= L_rows V_cols^T (8 FMAs per entry,
//      the tile stays in registers: only the panel rows move through LDS); the tiles of the panel
//      after next publish themselves once updated and leave the registers;
//   A  (before B of panel M+1) panel M's update of panel M+1's eight columns, in LDS, by every
//      thread: two entries of one row each, so it costs ~16 FMAs per thread instead of the
//      128 of a register tile's look-ahead in one wave (1.5k cycles per panel).
// Panel values are double-buffered (panel M+1 in one buffer while panel M+2 is published into the
// other) and so are L / V (panel M's are read by C while B writes panel M+1's).  Every entry sees
// the same updates in the same order as the register path: results are unchanged bit for bit.
// Two barriers per eight pivots.  The augmented row ends as y = D^-1 L^-1 b, and wave 0 solves
// L^T x = y.  Failure rule as the other kernels: an exactly zero pivot fails the solve.
// LDS: packed strictly-lower L (N(N-1)/2), two panel-value, two L and two V arrays ((Np+8) x 8
// each), y (N).
constexpr int kPW = 8;             // panel width (pivots per panel): 4 or 8
static_assert(kPW == 4 || kPW == 8, "panels of one or two tile columns");
constexpr int kTPP = kPW / 4;      // tile columns per panel
__host__ __device__ inline int ldlt_pan_rows(int N) { return ldlt_np4(N) + 8; }
// panel arrays: rows of kPW doubles in groups of four, each group padded by 2 doubles, so that
// the lanes of a wave reading different row groups spread over the LDS banks
constexpr int kPG = 4 * kPW + 2;
__host__ __device__ inline int ldlt_prow(int i) { return (i >> 2) * kPG + (i & 3) * kPW; }
__host__ __device__ inline int ldlt_pan_arr(int N) { return ldlt_pan_rows(N) / 4 * kPG; }
inline size_t ldlt_pan_smem(int N) {
  return ((size_t)N * (N - 1) / 2 + 6 * (size_t)ldlt_pan_arr(N) + N) * sizeof(double);
}
// (one tile per thread: with two the trailing update doubles and the panel kernel loses to the
// column-step one, e.g. 91 us at N = 126)
inline bool ldlt_pan_fits(int N) { return ldlt_pan_smem(N) <= kLdltColMaxSmem && ldlt_col_tiles(N) <= 512 && N < 128; }
// default where it fits (debug option ldlt = ORBX_BA_LDLT_COLUMN keeps the column-step kernel)
inline bool ldlt_use_pan(int N) { return ldlt_pan_fits(N) && ba_opts().ldlt == ORBX_BA_LDLT_AUTO; }
constexpr int ldlt_tri(int a, int b) { return a * (a + 1) / 2 + b; }

template <int TPT, int NT, int R>  // R: 64-row groups of the back solve (N < 64 R)
__device__ __forceinline__ void k_ba_ldlt_pan_body(const BaDev& D) {
  if (lm_skip(D) || !D.ldlt_pan) return;
  extern __shared__ __attribute__((aligned(16))) double Lpk[];  // row k: Lpk[k(k-1)/2 + c], c < k
  __shared__ int fail;
  const int N = 6 * D.nposes, tid = threadIdx.x;
  const int Np4 = ldlt_np4(N), Tr = Np4 / 4, Tc = (N + 3) / 4;
  const int ntiles = Tc * Tr - Tc * (Tc - 1) / 2;
  const int PA = ldlt_pan_arr(N);
  double* Pn = Lpk + (size_t)N * (N - 1) / 2;  // row i at ldlt_prow(i): current panel values
  double* Lp = Pn + PA;                         // panel L (scaled)
  double* Vp = Lp + PA;                         // panel V = L D (unscaled)
  double* ys = Vp + PA;                         // [N] y = D^-1 L^-1 b
  double* Lp2 = ys + N;                         // the second L / V set
  double* Vp2 = Lp2 + PA;
  double* Pn2 = Vp2 + PA;                       // the second panel-value buffer
  double a[TPT][4][4];
  int ti[TPT], tk[TPT];
  LDLT_TS(0);
  if (tid == 0) fail = 0;
#pragma unroll
  for (int t = 0; t < TPT; t++) {
    int x = tid + NT * t, k = 0;
    ti[t] = 0;
    tk[t] = -1;  // inactive
    if (x < ntiles) {
      while (x >= Tr - k) {  // column-major tile order
        x -= Tr - k;
        k++;
      }
      tk[t] = k;
      ti[t] = k + x;
    }
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int i = 4 * ti[t] + p, kk = 4 * tk[t] + q;
        double v = 0.0;
        if (tk[t] >= 0 && kk < N) v = i < N ? D.S[(size_t)i * N + kk] : (i == N ? D.bs[kk] : 0.0);
        a[t][p][q] = v;
      }
  }
  // (the tile loads above are in flight while the panel arrays are cleared)
  for (int j = tid; j < 3 * PA; j += NT) Pn[j] = 0.0;  // padding rows / columns stay finite
  for (int j = tid; j < 3 * PA; j += NT) Lp2[j] = 0.0;
  __syncthreads();
#pragma unroll
  for (int t = 0; t < TPT; t++) {  // panels 0 and 1 publish and leave the registers
    if (tk[t] >= 0 && tk[t] < 2 * kTPP) {
      double* P = tk[t] < kTPP ? Pn : Pn2;
#pragma unroll
      for (int p = 0; p < 4; p++) {
        double2_t* dst = reinterpret_cast<double2_t*>(P + ldlt_prow(4 * ti[t] + p) + 4 * (tk[t] % kTPP));
        dst[0] = double2_t{a[t][p][0], a[t][p][1]};
        dst[1] = double2_t{a[t][p][2], a[t][p][3]};
      }
    }
  }
  __syncthreads();
  LDLT_TS(1);
  // B: the panel rows of panel M into (Lq, Vq)
  auto panel_rows = [&](int M, const double* Pq, double* Lq, double* Vq) {
    constexpr int W = kPW, H = kPW / 2;  // (H: double2 per panel row)
    const int c0 = W * M, w = min(W, N - c0);
    const int i = c0 + tid;
    if (i <= N) {
      double Dm[W * (W + 1) / 2], u[W];
#pragma unroll
      for (int r = 0; r < W; r++) {
        const double2_t* src = reinterpret_cast<const double2_t*>(Pq + ldlt_prow(c0 + r));
        double row[W];
#pragma unroll
        for (int h = 0; h < H; h++) {
          const double2_t v = src[h];
          row[2 * h] = v.x, row[2 * h + 1] = v.y;
        }
#pragma unroll
        for (int c = 0; c <= r; c++) Dm[ldlt_tri(r, c)] = row[c];
      }
      {
        const double2_t* src = reinterpret_cast<const double2_t*>(Pq + ldlt_prow(i));
#pragma unroll
        for (int h = 0; h < H; h++) {
          const double2_t v = src[h];
          u[2 * h] = v.x, u[2 * h + 1] = v.y;
        }
      }
      double L[W], V[W];
      bool zero = false;
#pragma unroll
      for (int q = 0; q < W; q++) {
        L[q] = 0.0;
        V[q] = 0.0;
        if (q < w) {  // uniform
          const double d = Dm[ldlt_tri(q, q)];
          zero |= d == 0.0;
          const double rq = rcp_nr(d);
          double lq[W];
#pragma unroll
          for (int r = q + 1; r < W; r++) lq[r] = Dm[ldlt_tri(r, q)] * rq;
#pragma unroll
          for (int r = q + 1; r < W; r++)
#pragma unroll
            for (int c = q + 1; c <= r; c++) Dm[ldlt_tri(r, c)] = __builtin_fma(-lq[r], Dm[ldlt_tri(c, q)], Dm[ldlt_tri(r, c)]);
          V[q] = u[q];
          L[q] = u[q] * rq;
#pragma unroll
          for (int c = q + 1; c < W; c++) u[c] = __builtin_fma(-L[q], Dm[ldlt_tri(c, q)], u[c]);
        }
      }
      if (tid == 0 && zero) fail = 1;
      double2_t* lo = reinterpret_cast<double2_t*>(Lq + ldlt_prow(i));
      double2_t* vo = reinterpret_cast<double2_t*>(Vq + ldlt_prow(i));
#pragma unroll
      for (int h = 0; h < H; h++) {
        lo[h] = double2_t{L[2 * h], L[2 * h + 1]};
        vo[h] = double2_t{V[2 * h], V[2 * h + 1]};
      }
      if (i < N) {
        double* lrow = Lpk + (size_t)i * (i - 1) / 2 + c0;
#pragma unroll
        for (int q = 0; q < W; q++)
          if (c0 + q < i && q < w) lrow[q] = L[q];
      } else {
#pragma unroll
        for (int q = 0; q < W; q++)
          if (q < w) ys[c0 + q] = L[q];
      }
    }
  };
  // C: the register tiles right of panel M+1 take A -= L_rows V_cols^T; those of panel M+2 then
  // publish themselves into Pq and retire
  auto trailing = [&](int M, const double* Lq, const double* Vq, double* Pq) {
#pragma unroll
    for (int t = 0; t < TPT; t++) {
      if (tk[t] >= kTPP * (M + 2)) {
        const double* lr = Lq + kPG * ti[t];
        const double* vr = Vq + kPG * tk[t];
#pragma unroll
        for (int h = 0; h < kTPP; h++) {
          double Lv[4][4], Vv[4][4];
#pragma unroll
          for (int p = 0; p < 4; p++) {
            const double2_t* ls = reinterpret_cast<const double2_t*>(lr + kPW * p + 4 * h);
            const double2_t* vs = reinterpret_cast<const double2_t*>(vr + kPW * p + 4 * h);
            const double2_t l0 = ls[0], l1 = ls[1], v0 = vs[0], v1 = vs[1];
            Lv[p][0] = l0.x, Lv[p][1] = l0.y, Lv[p][2] = l1.x, Lv[p][3] = l1.y;
            Vv[p][0] = v0.x, Vv[p][1] = v0.y, Vv[p][2] = v1.x, Vv[p][3] = v1.y;
          }
#pragma unroll
          for (int s = 0; s < 4; s++)
#pragma unroll
            for (int p = 0; p < 4; p++)
#pragma unroll
              for (int q = 0; q < 4; q++) a[t][p][q] = __builtin_fma(-Lv[p][s], Vv[q][s], a[t][p][q]);
        }
        if (tk[t] < kTPP * (M + 3)) {  // panel M+2 publishes itself
#pragma unroll
          for (int p = 0; p < 4; p++) {
            double2_t* dst = reinterpret_cast<double2_t*>(Pq + ldlt_prow(4 * ti[t] + p) + 4 * (tk[t] % kTPP));
            dst[0] = double2_t{a[t][p][0], a[t][p][1]};
            dst[1] = double2_t{a[t][p][2], a[t][p][3]};
          }
        }
      }
    }
  };
  // A: panel M's update of panel M+1's values in Pq (rows c1 = kPW (M+1) .. N, kPW columns):
  // thread -> (row c1 + tid / 4, columns CPT (tid % 4) .. +CPT-1), the s = 0..kPW-1 FMAs in the
  // register path's order
  auto lookahead = [&](const double* Lq, const double* Vq, double* Pq, int c1) {
    constexpr int CPT = kPW / 4;
    const int i = c1 + tid / 4, j0 = CPT * (tid & 3);
    if (i <= N) {
      const double2_t* ls = reinterpret_cast<const double2_t*>(Lq + ldlt_prow(i));
      double* dst = Pq + ldlt_prow(i) + j0;
      double x[CPT];
      const double2_t* vr[CPT];
#pragma unroll
      for (int c = 0; c < CPT; c++) {
        x[c] = dst[c];
        vr[c] = reinterpret_cast<const double2_t*>(Vq + ldlt_prow(c1 + j0 + c));
      }
#pragma unroll
      for (int h = 0; h < kPW / 2; h++) {
        const double2_t l = ls[h];
        double2_t v[CPT];
#pragma unroll
        for (int c = 0; c < CPT; c++) v[c] = vr[c][h];
#pragma unroll
        for (int c = 0; c < CPT; c++) x[c] = __builtin_fma(-l.x, v[c].x, x[c]);
#pragma unroll
        for (int c = 0; c < CPT; c++) x[c] = __builtin_fma(-l.y, v[c].y, x[c]);
      }
#pragma unroll
      for (int c = 0; c < CPT; c++) dst[c] = x[c];
    }
  };
  static_assert(NT / 4 >= 124, "one look-ahead pass covers rows kPW .. N of a panel (N < 128)");
  panel_rows(0, Pn, Lp, Vp);
  __syncthreads();
  for (int M = 0; kTPP * M < Tc; M++) {
    double* Lc = (M & 1) ? Lp2 : Lp;  // panel M's L / V
    double* Vc = (M & 1) ? Vp2 : Vp;
    double* Pnext = (M & 1) ? Pn : Pn2;  // panel M+1's values (then panel M+3's)
    double* Pafter = (M & 1) ? Pn2 : Pn;  // panel M+2's values, published by C below
    const bool more = kTPP * (M + 1) < Tc;
    if (more) lookahead(Lc, Vc, Pnext, kPW * (M + 1));
    __syncthreads();
    LDLT_TS(2 + 2 * M);
    if (more) panel_rows(M + 1, Pnext, (M & 1) ? Lp : Lp2, (M & 1) ? Vp : Vp2);
    LDLT_TS(32 + M);  // (thread 0 is always a panel-row thread: the rows' chain ends here)
    trailing(M, Lc, Vc, Pafter);
    __syncthreads();
    LDLT_TS(3 + 2 * M);
  }
  if (fail) {
    if (tid == 0) D.scal[2] = 0.0;
    return;
  }
  if (tid >= 64) return;
  // L^T x = y one row at a time from the bottom: x_k = y_k (final once every row below is done) is
  // read out of its lane and each lane takes y_i -= L[k][i] x_k for its rows i < k.  Per row the
  // dependent chain is one lane read and one FMA; rows are loaded eight ahead (the lgkmcnt window
  // is 15) and the reads run past row k's k entries into the next rows or the panel arrays
  // (written LDS): they are masked where they are used -- a select right after a load would wait
  // for it there -- and the loops have no branches, so the waits stay per group of eight rows.
  // Two phases by the 64-row group of k, so that each row needs no select of its y register and
  // phase 2 (k < 64) leaves the upper group alone.
  // (The 8-row blocked form -- readlanes of a block, an 8x8 unit triangular solve, two register
  // sets of 44 LDS reads -- took 1.5k cycles per block, 24k of the kernel's 100k at N = 120.)
  const int lane = tid;
  double y[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int i = lane + 64 * r;
    y[r] = i < N ? ys[i] : 0.0;
  }
  static_assert(R == 2, "the two-phase row loop below: rows 64.. then 0..63");
  // Rows are clamped to [1, N-1]: a row k >= N (the 8-row groups round N up) reads row N-1's
  // entries, which are finite and meet x_k = y_k = 0, and no read leaves the kernel's LDS (the
  // lanes past a row's k entries read the next rows or the zero-initialised panel arrays).
  auto row_ptr = [&](int k) {
    const int r = min(max(k, 1), max(N - 1, 1));
    return Lpk + (size_t)r * (r - 1) / 2;
  };
  constexpr int kAhead = 8;  // rows loaded ahead (<= 15 LDS reads in flight)
  LDLT_TS(48);
  // phase 1 (N > 64): rows k = K1 .. 64 (K1 >= N - 1; rows k >= N have x_k = y_k = 0 and change
  // nothing): x_k sits in y[1]; rows i < 64 always take the update, rows i >= 64 only when i < k
  if (N > 64) {
    const int K1 = 64 + 8 * ((N - 64 + 7) / 8) - 1;
    double L0[kAhead], L1[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; u++) {
      const double* Lk = row_ptr(K1 - u);
      L0[u] = Lk[lane];
      L1[u] = Lk[lane + 64];
    }
    for (int k0 = K1; k0 >= 64; k0 -= kAhead) {
#pragma unroll
      for (int u = 0; u < kAhead; u++) {
        const int k = k0 - u;
        const double xk = readlane_d(y[1], k - 64);
        y[0] = __builtin_fma(-L0[u], xk, y[0]);
        const double y1 = __builtin_fma(-L1[u], xk, y[1]);
        y[1] = lane + 64 < k ? y1 : y[1];  // (rows at or past k keep their value: no 0 * inf)
        const double* Lk = row_ptr(k - kAhead);  // (rows below 64 of the next group: unused)
        L0[u] = Lk[lane];
        L1[u] = Lk[lane + 64];
      }
    }
  }
  // phase 2: rows k = K2 .. 0 (K2 = min(63, N - 1) rounded up to a group of eight), x_k in y[0];
  // rows i >= 64 are final
  {
    const int K2 = min(63, 8 * ((N + 7) / 8) - 1);
    double L0[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; u++) L0[u] = row_ptr(K2 - u)[lane];
    for (int k0 = K2; k0 >= 0; k0 -= kAhead) {
#pragma unroll
      for (int u = 0; u < kAhead; u++) {
        const int k = k0 - u;
        const double xk = readlane_d(y[0], k);
        const double y0 = __builtin_fma(-L0[u], xk, y[0]);
        y[0] = lane < k ? y0 : y[0];
        L0[u] = row_ptr(k - kAhead)[lane];  // (k - kAhead < 1: unused)
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; r++)
    if (lane + 64 * r < N) D.xp[lane + 64 * r] = y[r];
  if (lane == 0) D.scal[2] = 1.0;
  LDLT_TS(63);
}
template <int TPT, int NT, int R>
__global__ __launch_bounds__(NT) void k_ba_ldlt_pan(BaDev D) { k_ba_ldlt_pan_body<TPT, NT, R>(D); }
template <int TPT, int NT, int R>
__global__ __launch_bounds__(NT) void k_ba_ldlt_pan_many(const BaDev* __restrict__ Ds) {
  k_ba_ldlt_pan_body<TPT, NT, R>(Ds[blockIdx.z]);
}

// ---- reduced camera system beyond one workgroup: 64-wide panels over many workgroups ----
// k_ba_ldlt_tiled_*: the same right-looking LDL^T without pivoting, for the systems of a global map
// (GlobalBundleAdjustemnt: N up to kTiledMaxN = 3072, a 75 MB matrix that no single workgroup should
// walk).  The work matrix A lives in D.Sw: Nr = Np + 16 rows of Np doubles, Np = N padded to a
// multiple of 64 with an identity block (decoupled, never a zero pivot); row Np is the augmented
// row b^T (rows Np+1 .. Np+15 are zero: the row tiles stay 16 high), so the forward solve rides on
// the factorisation as in k_ba_ldlt_col.  Entries are kept unscaled, W = L D.  Per panel j0, three
// launches ordered by the stream alone:
//   diag   one workgroup: the 64 x 64 diagonal block in LDS, one barrier per pivot; W11 back into A,
//          L11 and 1 / d into the panel scratch;
//   strip  32 rows below the panel per workgroup: W21 L11^T = A21 solved in LDS (W21 back into A,
//          L21 = W21 D^-1 into the panel scratch Lp);
//   trail  A22 -= W21 L21^T, one 64 x 64 block of the lower triangle per workgroup, FP64 MFMA
//          16x16x4 tiles with k_ba_ldlt's operand layout (K = 64: sixteen steps per tile).
// The augmented row then holds z = L^-1 b, and L^T x = D^-1 z is solved from the last panel up, one
// launch per panel (back): every workgroup solves the panel's 64 unknowns for itself (the same
// instructions on the same inputs: the same bits) and takes v_i -= sum_c W_ci x_c for its own 256
// rows i above the panel, in z's place; x_i = v_i / d_i.  No block waits for another.  Partitions
// and summation orders are fixed, nothing is accumulated atomically: results are identical from run
// to run.  Failure rule as the other kernels: an exactly zero pivot fails the solve; the diag
// launch that meets it clears scal[2] (load set it), and every later launch of that solve returns
// at once on reading it.
constexpr int kTB = 64;                  // panel width
constexpr int kTiledMaxPoses = 512;      // free keyframes of the largest system
constexpr int kTiledMaxN = 6 * kTiledMaxPoses;
constexpr int kTiledStripRows = 32;      // rows per workgroup of the strip solve
constexpr int kTiledNT = 256;
inline int ldlt_tiled_np(int N) { return (N + kTB - 1) / kTB * kTB; }
// D.Sw of the tiled kernels, in doubles: A (Nr x Np) | Lp (Nr x 64) | L11 (64 x 64) | 1/d (64)
inline size_t ldlt_tiled_doubles(int N) {
  const size_t Np = ldlt_tiled_np(N), Nr = Np + 16;
  return Nr * Np + Nr * kTB + kTB * kTB + kTB;
}
struct TiledWs {
  double *A, *Lp, *L11, *dinv;
  int N, Np, Nr;
};
__device__ inline TiledWs tiled_ws(const BaDev& D) {
  TiledWs w;
  w.N = 6 * D.nposes;
  w.Np = (w.N + kTB - 1) / kTB * kTB;
  w.Nr = w.Np + 16;
  w.A = D.Sw;
  w.Lp = w.A + (size_t)w.Nr * w.Np;
  w.L11 = w.Lp + (size_t)w.Nr * kTB;
  w.dinv = w.L11 + kTB * kTB;
  return w;
}

__global__ __launch_bounds__(kTiledNT) void k_ba_ldlt_tiled_load(BaDev D) {
  if (lm_skip(D)) return;
  const TiledWs w = tiled_ws(D);
  const size_t total = (size_t)w.Nr * w.Np;
  for (size_t idx = (size_t)blockIdx.x * kTiledNT + threadIdx.x; idx < total; idx += (size_t)gridDim.x * kTiledNT) {
    const int r = (int)(idx / w.Np), c = (int)(idx - (size_t)r * w.Np);
    double v = 0.0;
    if (r < w.N)
      v = c < w.N ? D.S[(size_t)r * w.N + c] : 0.0;
    else if (r < w.Np)
      v = r == c ? 1.0 : 0.0;
    else if (r == w.Np)
      v = c < w.N ? D.bs[c] : 0.0;
    w.A[idx] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) D.scal[2] = 1.0;
}

__global__ __launch_bounds__(kTiledNT) void k_ba_ldlt_tiled_diag(BaDev D, int j0) {
  if (lm_skip(D) || D.scal[2] == 0.0) return;
  const TiledWs w = tiled_ws(D);
  __shared__ double T[kTB][kTB + 1];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < kTB * kTB; idx += kTiledNT) {
    const int r = idx >> 6, c = idx & 63;
    T[r][c] = w.A[(size_t)(j0 + r) * w.Np + j0 + c];
  }
  __syncthreads();
  for (int c = 0; c < kTB; c++) {
    const double d = T[c][c];  // (final: every update of column c is behind the last barrier)
    if (d == 0.0) {            // uniform
      if (tid == 0) D.scal[2] = 0.0;
      return;
    }
    const double invd = 1.0 / d;
    for (int idx = tid; idx < kTB * kTB; idx += kTiledNT) {
      const int r = idx >> 6, k = idx & 63;
      if (k > c && k <= r) T[r][k] -= T[r][c] * invd * T[k][c];  // column c is not written in step c
    }
    __syncthreads();
  }
  for (int idx = tid; idx < kTB * kTB; idx += kTiledNT) {
    const int r = idx >> 6, c = idx & 63;
    if (c <= r) w.A[(size_t)(j0 + r) * w.Np + j0 + c] = T[r][c];
    w.L11[idx] = c < r ? T[r][c] * (1.0 / T[c][c]) : (c == r ? 1.0 : 0.0);
  }
  if (tid < kTB) w.dinv[tid] = 1.0 / T[tid][tid];
}

__global__ __launch_bounds__(kTiledNT) void k_ba_ldlt_tiled_strip(BaDev D, int j0) {
  if (lm_skip(D) || D.scal[2] == 0.0) return;
  const TiledWs w = tiled_ws(D);
  __shared__ double Ls[kTB][kTB + 1];
  __shared__ double T[kTiledStripRows][kTB + 1];
  __shared__ double dinv[kTB];
  const int tid = threadIdx.x;
  const int i0 = j0 + kTB + kTiledStripRows * blockIdx.x;  // the workgroup's first row
  for (int idx = tid; idx < kTB * kTB; idx += kTiledNT) Ls[idx >> 6][idx & 63] = w.L11[idx];
  if (tid < kTB) dinv[tid] = w.dinv[tid];
  for (int idx = tid; idx < kTiledStripRows * kTB; idx += kTiledNT) {
    const int r = idx >> 6, c = idx & 63;
    T[r][c] = i0 + r < w.Nr ? w.A[(size_t)(i0 + r) * w.Np + j0 + c] : 0.0;
  }
  __syncthreads();
  // W21 L11^T = A21, right-looking: after step m every entry right of column m has taken W_rm L11_cm
  for (int m = 0; m + 1 < kTB; m++) {
    for (int idx = tid; idx < kTiledStripRows * kTB; idx += kTiledNT) {
      const int r = idx >> 6, c = idx & 63;
      if (c > m) T[r][c] -= T[r][m] * Ls[c][m];
    }
    __syncthreads();
  }
  for (int idx = tid; idx < kTiledStripRows * kTB; idx += kTiledNT) {
    const int r = idx >> 6, c = idx & 63;
    if (i0 + r < w.Nr) {
      w.A[(size_t)(i0 + r) * w.Np + j0 + c] = T[r][c];
      w.Lp[(size_t)(i0 + r) * kTB + c] = T[r][c] * dinv[c];
    }
  }
}

__global__ __launch_bounds__(kTiledNT) void k_ba_ldlt_tiled_trail(BaDev D, int j0) {
  if (lm_skip(D) || D.scal[2] == 0.0) return;
  const int bi = blockIdx.x, bk = blockIdx.y;
  if (bk > bi) return;  // the lower triangle of 64 x 64 blocks
  const TiledWs w = tiled_ws(D);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int R0 = j0 + kTB + kTB * bi + 16 * wv, Cb = j0 + kTB + kTB * bk;
  if (R0 >= w.Nr) return;  // (the augmented block row is one tile high)
  const size_t ld = w.Np;
  double4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int kk = 0; kk < kTB / 4; kk++) {
    const double av = w.A[(size_t)(R0 + (lane & 15)) * ld + j0 + 4 * kk + (lane >> 4)];  // W[row][k]
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const double bv = w.Lp[(size_t)(Cb + 16 * t + (lane & 15)) * kTB + 4 * kk + (lane >> 4)];  // L[col][k]
      acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
      const size_t o = (size_t)(R0 + (lane >> 4) + 4 * rr) * ld + Cb + 16 * t + (lane & 15);
      w.A[o] -= acc[t][rr];
    }
}

__global__ __launch_bounds__(kTiledNT) void k_ba_ldlt_tiled_back(BaDev D, int j0) {
  if (lm_skip(D) || D.scal[2] == 0.0) return;
  const TiledWs w = tiled_ws(D);
  __shared__ double T[kTB][kTB + 1];
  __shared__ double xs[kTB];
  const int tid = threadIdx.x;
  double* v = w.A + (size_t)w.Np * w.Np;  // the augmented row: z, then z minus the solved panels' terms
  for (int idx = tid; idx < kTB * kTB; idx += kTiledNT) {
    const int r = idx >> 6, c = idx & 63;
    T[r][c] = w.A[(size_t)(j0 + r) * w.Np + j0 + c];
  }
  __syncthreads();
  if (tid < 64) {  // wave 0: lane r holds v_r; x_c = v_c / d_c from the bottom up
    const int r = tid;
    double val = v[j0 + r], x = 0.0;
    const double invd = 1.0 / T[r][r];
#pragma unroll
    for (int c = kTB - 1; c >= 0; c--) {
      const double xc = readlane_d(val * invd, c);
      if (r < c) val -= T[c][r] * xc;
      if (r == c) x = xc;
    }
    xs[r] = x;
    if (blockIdx.x == 0 && j0 + r < w.N) D.xp[j0 + r] = x;
  }
  __syncthreads();
  const int i = blockIdx.x * kTiledNT + tid;
  if (i < j0) {
    double acc = v[i];
    for (int c = 0; c < kTB; c++) acc -= w.A[(size_t)(j0 + c) * w.Np + i] * xs[c];
    v[i] = acc;
  }
}

// The launches of one tiled solve, in stream order.
inline void ldlt_tiled_launch(const BaDev& D, hipStream_t st) {
  const int N = 6 * D.nposes, Np = ldlt_tiled_np(N), Nr = Np + 16;
  const size_t total = (size_t)Nr * Np;
  const int gl = (int)std::min<size_t>((total + kTiledNT - 1) / kTiledNT, 4096);
  hipLaunchKernelGGL(k_ba_ldlt_tiled_load, dim3(gl), dim3(kTiledNT), 0, st, D);
  for (int j0 = 0; j0 < Np; j0 += kTB) {
    hipLaunchKernelGGL(k_ba_ldlt_tiled_diag, dim3(1), dim3(kTiledNT), 0, st, D, j0);
    const int rows = Nr - j0 - kTB;  // below the panel, the augmented tile row included
    hipLaunchKernelGGL(k_ba_ldlt_tiled_strip, dim3((rows + kTiledStripRows - 1) / kTiledStripRows), dim3(kTiledNT), 0,
                       st, D, j0);
    const int mc = (Np - j0 - kTB) / kTB;  // 64 x 64 block columns right of the panel
    if (mc > 0) hipLaunchKernelGGL(k_ba_ldlt_tiled_trail, dim3(mc + 1, mc), dim3(kTiledNT), 0, st, D, j0);
  }
  for (int j0 = Np - kTB; j0 >= 0; j0 -= kTB)
    hipLaunchKernelGGL(k_ba_ldlt_tiled_back, dim3(std::max((j0 + kTiledNT - 1) / kTiledNT, 1)), dim3(kTiledNT), 0, st,
                       D, j0);
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device), raised only when a larger
// size is asked for: the runtime call costs microseconds and used to sit between the launches of
// every LM phase (the device idled behind it)
inline hipError_t set_smem_attr(const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lk(mu);
  size_t& have = done[{fn, dev}];
  if (bytes <= have) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) have = bytes;
  return e;
}

// Launch plan for the reduced system: the 8-wide panel kernel (N < 128), the column-step kernel while
// the packed factor fits LDS, else the 16-wide blocked MFMA kernel (LDS or global) up to a padded size
// of kLdltMaxNp, and the tiled kernels beyond it (up to kTiledMaxN).  The debug options
// (orbx_debug_ba_options) can force the column-step or the blocked kernel where they fit, and the
// tiled kernels at any size, for tests.
struct LdltPlan {
  int N = 0, tpt = 0, nt = 1024;
  bool col = false, in_lds = false, pan = false, tiled = false;
  size_t smem = 0;
  // the tiled kernels: beyond the single-workgroup kernels' size, or forced (tests run them small)
  static bool use_tiled(int N) {
    const int o = ba_opts().ldlt;
    return (o == ORBX_BA_LDLT_TILED && N >= 6) || (o == ORBX_BA_LDLT_AUTO && ldlt_np(N) > kLdltMaxNp);
  }
  // doubles of D.Sw the chosen kernel needs (0: none)
  size_t sw_doubles() const {
    if (tiled) return ldlt_tiled_doubles(N);
    return !col && !pan && !in_lds ? (size_t)ldlt_np(N) * ldlt_np(N) : 0;
  }
  hipError_t prepare(int n, bool allow_pan = true) {
    N = n;
    tiled = use_tiled(N);
    if (tiled) {  // static LDS only
      pan = col = in_lds = false;
      if (N > kTiledMaxN) return hipErrorInvalidValue;
      smem = 0;
      return hipSuccess;
    }
    pan = allow_pan && ldlt_use_pan(N);
    if (pan) {
      col = false;
      in_lds = true;
      nt = 512;
      tpt = 1;
      smem = ldlt_pan_smem(N);
      return set_smem_attr(kernel_ptr(), smem);
    }
    col = ldlt_col_fits(N) && ba_opts().ldlt != ORBX_BA_LDLT_BLOCKED;
    if (col) {
      nt = kLdltColNT;
      // ldlt_col_fits: at most kLdltColMaxTiles = 2 * kLdltColNT tiles, so one or two per thread
      static_assert(kLdltColMaxTiles <= 2 * kLdltColNT, "k_ba_ldlt_col is instantiated for TPT = 1 and 2 only");
      tpt = ldlt_col_tiles(N) <= kLdltColNT ? 1 : 2;
      smem = ldlt_col_smem(N);
    } else {
      in_lds = ldlt_np(N) <= kLdltLdsNp;
      smem = ldlt_smem_bytes(N, in_lds);
    }
    return set_smem_attr(kernel_ptr(), smem);
  }
  const void* kernel_ptr() const {
    if (pan) return (const void*)k_ba_ldlt_pan<1, 512, 2>;
    if (col) return tpt == 1 ? (const void*)k_ba_ldlt_col<1, kLdltColNT> : (const void*)k_ba_ldlt_col<2, kLdltColNT>;
    return in_lds ? (const void*)k_ba_ldlt<true> : (const void*)k_ba_ldlt<false>;
  }
  // batched driver: the panel or the column-step kernel over K problems (blockIdx.z), sized for the
  // largest (the blocked kernel has no batched form: optimize_many refuses such a batch)
  const void* many_ptr() const {
    if (pan) return (const void*)k_ba_ldlt_pan_many<1, 512, 2>;
    return tpt == 1 ? (const void*)k_ba_ldlt_col_many<1, kLdltColNT> : (const void*)k_ba_ldlt_col_many<2, kLdltColNT>;
  }
  hipError_t prepare_many() const {
    return set_smem_attr(many_ptr(), smem);
  }
  void launch_many(const BaDev* Ds, int K, hipStream_t st) const {
    hipLaunchKernelGGL(reinterpret_cast<void (*)(const BaDev*)>(const_cast<void*>(many_ptr())), dim3(1, 1, K),
                       dim3(nt), smem, st, Ds);
  }
  void launch(const BaDev& D, hipStream_t st, int stage_limit = 99) const {
    if (tiled) {
      ldlt_tiled_launch(D, st);
    } else if (col || pan) {
      hipLaunchKernelGGL(reinterpret_cast<void (*)(BaDev)>(const_cast<void*>(kernel_ptr())), dim3(1), dim3(nt),
                         smem, st, D);
    } else if (in_lds) {
      hipLaunchKernelGGL(k_ba_ldlt<true>, dim3(1), dim3(1024), smem, st, D, stage_limit);
    } else {
      hipLaunchKernelGGL(k_ba_ldlt<false>, dim3(1), dim3(1024), smem, st, D, stage_limit);
    }
  }
};

}  // namespace orbx

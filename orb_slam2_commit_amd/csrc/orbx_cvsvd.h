// orbx_cvsvd.h -- OpenCV 3.2's Jacobi SVD (modules/core/src/lapack.cpp: JacobiSVDImpl_, SVBkSbImpl_) and
// cv::RNG::next, restated once for every unit that calls cv::SVD / cvSVD / cvInvert / cvSolve: pnp.hip
// at T = double (EPnP; oracle/pnp.cpp is its yardstick) and initializer.hip at T = float
// (tests/initializer_literal.py).  The library's template has one text for both scalars and so has this
// one: W, the dot products and the rotation's angle are double whatever T is; the rows, c, s and the
// rotated elements are T.  Every cast below is the library's (at T = double they are no-ops), every sum
// runs in the library's order, and -ffp-contract=off keeps the products unfused: nothing here may be
// re-associated.  __host__ __device__: the Initializer's host build (orbx_debug_initializer_host) runs
// the same text.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

namespace orbx {
namespace cvsvd {

#define CVSVD_HD __host__ __device__ __forceinline__

// cv::RNG::next (multiply-with-carry)
struct CvRng {
  unsigned long long state;
  CVSVD_HD unsigned next() {
    state = (unsigned long long)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
    return (unsigned)state;
  }
};

// JacobiSVDImpl_'s two constants per scalar: minval, and eps in the scalar's own type
template <class T> struct Lim;
template <> struct Lim<float> {
  static constexpr double minval = FLT_MIN;
  static constexpr float eps = FLT_EPSILON * 2;
};
template <> struct Lim<double> {
  static constexpr double minval = DBL_MIN;
  static constexpr double eps = DBL_EPSILON * 10;
};
CVSVD_HD float abs_t(float x) { return __builtin_fabsf(x); }
CVSVD_HD double abs_t(double x) { return __builtin_fabs(x); }

// One Jacobi rotation of rows i < j of At (N rows of length M, row stride M; W the squared row norms;
// Vt N x N, row stride N).  Returns false when the pair is already orthogonal (skipped).  kV = false
// skips V's arithmetic only: it never feeds back into At or W.
template <class T, int M, int N, bool kV>
CVSVD_HD bool jacobi_rotate(T* At, double* W, T* Vt, int i, int j) {
  const T eps = Lim<T>::eps;
  T* Ai = At + i * M;
  T* Aj = At + j * M;
  double a = W[i], p = 0, b = W[j];
  T xi[M], xj[M];
#pragma unroll
  for (int k = 0; k < M; k++) {
    xi[k] = Ai[k];
    xj[k] = Aj[k];
  }
#pragma unroll
  for (int k = 0; k < M; k++) p += (double)xi[k] * (double)xj[k];
  if (__builtin_fabs(p) <= (double)eps * __builtin_sqrt(a * b)) return false;
  p *= 2;
  const double beta = a - b, gamma = __builtin_sqrt(p * p + beta * beta);
  T c, s;
  if (beta < 0) {
    const double delta = (gamma - beta) * 0.5;
    s = (T)__builtin_sqrt(delta / gamma);
    c = (T)(p / (gamma * (double)s * 2));
  } else {
    c = (T)__builtin_sqrt((gamma + beta) / (gamma * 2));
    s = (T)(p / (gamma * (double)c * 2));
  }
  a = b = 0;
#pragma unroll
  for (int k = 0; k < M; k++) {
    const T t0 = c * xi[k] + s * xj[k];
    const T t1 = -s * xi[k] + c * xj[k];
    Ai[k] = t0;
    Aj[k] = t1;
    a += (double)t0 * (double)t0;
    b += (double)t1 * (double)t1;
  }
  W[i] = a;
  W[j] = b;
  if (kV) {
    T* Vi = Vt + i * N;
    T* Vj = Vt + j * N;
#pragma unroll
    for (int k = 0; k < N; k++) {
      const T t0 = c * Vi[k] + s * Vj[k];
      const T t1 = -s * Vi[k] + c * Vj[k];
      Vi[k] = t0;
      Vj[k] = t1;
    }
  }
  return true;
}

template <class T>
CVSVD_HD void swap_t(T& a, T& b) {
  const T t = a;
  a = b;
  b = t;
}

// After the sweeps: singular values, descending sort (rows of At and Vt swapped along), then the
// cv::RNG(0x12345678) completion and normalisation of the first N1 rows (the library's n1: 0 skips it,
// N1 > N makes rows N .. N1-1 of At, which must exist, out of nothing).  W is left holding the sorted
// singular values; with kSmall they are copied to Wout (see jacobi_svd).  kUnroll: the row loops are
// unrolled (kSmall needs it: static indices; the wave form takes it for its lane 0's straight-line code).
template <class T, int M, int N, int N1, bool kV, bool kSmall, bool kUnroll = kSmall>
CVSVD_HD void jacobi_tail(T* At, double* W, double* Wout, T* Vt) {
  static_assert(kUnroll || !kSmall, "register matrices need static row indices");
  const double minval = Lim<T>::minval;
  const T eps = Lim<T>::eps;
  // rolled row loops work a row at a time (unrolled, the Initializer's 16x9 system issues all its loads
  // at once and the kernel's registers treble)
  constexpr int kRows = kUnroll ? N : 1, kRows1 = kUnroll ? N1 : 1;
#pragma unroll kRows
  for (int i = 0; i < N; i++) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < M; k++) {
      const T t = At[i * M + k];
      sd += (double)t * (double)t;
    }
    W[i] = __builtin_sqrt(sd);
  }
#pragma unroll kRows
  for (int i = 0; i < N - 1; i++) {
    int j = i;
#pragma unroll kRows
    for (int k = i + 1; k < N; k++)
      if (W[j] < W[k]) j = k;
    if (i != j) {
      if constexpr (kSmall) {  // W[j] with j runtime: select chains keep W in registers
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < N; k++)
          if (k == j) wj = W[k];
#pragma unroll
        for (int k = i + 1; k < N; k++)
          if (k == j) W[k] = W[i];
        W[i] = wj;
      } else {
        swap_t(W[i], W[j]);
      }
      if constexpr (kSmall) {  // rows of register arrays: swap with every candidate row under a
                               // select (static indices), never a runtime-indexed (scratch) access
#pragma unroll
        for (int r = i + 1; r < N; r++) {
          const bool sw = r == j;
#pragma unroll
          for (int k = 0; k < M; k++) {
            const T a = At[i * M + k], b = At[r * M + k];
            At[i * M + k] = sw ? b : a;
            At[r * M + k] = sw ? a : b;
          }
          if (kV) {
#pragma unroll
            for (int k = 0; k < N; k++) {
              const T a = Vt[i * N + k], b = Vt[r * N + k];
              Vt[i * N + k] = sw ? b : a;
              Vt[r * N + k] = sw ? a : b;
            }
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < M; k++) swap_t(At[i * M + k], At[j * M + k]);
        if (kV) {
#pragma unroll
          for (int k = 0; k < N; k++) swap_t(Vt[i * N + k], Vt[j * N + k]);
        }
      }
    }
  }
  if (kSmall) {
#pragma unroll
    for (int i = 0; i < N; i++) Wout[i] = W[i];
  }
  CvRng rng{0x12345678};
#pragma unroll kRows1
  for (int i = 0; i < N1; i++) {
    double sd = i < N ? W[i] : 0;
    for (int ii = 0; ii < 100 && sd <= minval; ii++) {
      // a zero singular value: a +-1/M vector, projected off the earlier rows twice, normalised
      const T val0 = (T)(1. / M);
#pragma unroll
      for (int k = 0; k < M; k++) At[i * M + k] = (rng.next() & 256) != 0 ? val0 : -val0;
      for (int iter = 0; iter < 2; iter++)
        for (int j = 0; j < i; j++) {
          sd = 0;
#pragma unroll
          for (int k = 0; k < M; k++) sd += (double)(At[i * M + k] * At[j * M + k]);
          T asum = 0;
#pragma unroll
          for (int k = 0; k < M; k++) {
            const T t = (T)((double)At[i * M + k] - sd * (double)At[j * M + k]);
            At[i * M + k] = t;
            asum += abs_t(t);
          }
          asum = asum > eps * (T)100 ? 1 / asum : 0;
#pragma unroll
          for (int k = 0; k < M; k++) At[i * M + k] *= asum;
        }
      sd = 0;
#pragma unroll
      for (int k = 0; k < M; k++) {
        const T t = At[i * M + k];
        sd += (double)t * (double)t;
      }
      sd = __builtin_sqrt(sd);
    }
    const T s = (T)(sd > minval ? 1 / sd : 0.);
#pragma unroll
    for (int k = 0; k < M; k++) At[i * M + k] *= s;
  }
}

// JacobiSVDImpl_<T> on N rows of length M in At (row stride M), one thread: on exit the first N1 rows
// of At are the left singular vectors (descending singular values in Wout, as doubles: a caller that
// wants the library's _Tp copy casts them), Vt the right ones.  Sizes are compile-time so the element
// loops unroll.  kSmall: W works in registers, the pair loops are unrolled and row swaps are selects,
// so that an At / Vt in registers never sees a run-time index (which would send it to scratch memory);
// without it W works in Wout and the pair loops stay rolled, for matrices in LDS or on the stack.
template <class T, int M, int N, int N1, bool kV, bool kSmall>
CVSVD_HD void jacobi_svd(T* At, double* Wout, T* Vt) {
  double Wreg[kSmall ? N : 1];
  double* W = kSmall ? Wreg : Wout;
  constexpr int max_iter = M > 30 ? M : 30;
  constexpr int kRows = kSmall ? N : 1;  // (see jacobi_tail)
#pragma unroll kRows
  for (int i = 0; i < N; i++) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < M; k++) {
      const T t = At[i * M + k];
      sd += (double)t * (double)t;
    }
    W[i] = sd;
    if (kV) {
#pragma unroll
      for (int k = 0; k < N; k++) Vt[i * N + k] = 0;
      Vt[i * N + i] = 1;
    }
  }
  for (int iter = 0; iter < max_iter; iter++) {
    bool changed = false;
    if constexpr (kSmall) {
#pragma unroll
      for (int i = 0; i < N - 1; i++)
#pragma unroll
        for (int j = i + 1; j < N; j++) changed |= jacobi_rotate<T, M, N, kV>(At, W, Vt, i, j);
    } else {
#pragma unroll 1
      for (int i = 0; i < N - 1; i++)
#pragma unroll 1
        for (int j = i + 1; j < N; j++) changed |= jacobi_rotate<T, M, N, kV>(At, W, Vt, i, j);
    }
    if (!changed) break;
  }
  jacobi_tail<T, M, N, N1, kV, kSmall>(At, W, Wout, Vt);
}

// The same SVD (no V, N1 = N) run by one wave on LDS data: rotation (i, j) only touches rows i, j, and
// in the cyclic order each row's rotations come in increasing i + j, so step t = i + j runs every pair
// (lane i, t - i) at once -- disjoint rows, each row's rotations in the reference order, so the result
// is bit-identical -- 2N-3 steps per sweep instead of N(N-1)/2.  The sort and null-row completion stay
// on lane 0.  Device only.
template <class T, int M, int N>
__device__ __forceinline__ void jacobi_svd_wave(T* At, double* W) {
  constexpr int max_iter = M > 30 ? M : 30;
  const int lane = threadIdx.x & 63;
  if (lane < N) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < M; k++) {
      const T t = At[lane * M + k];
      sd += (double)t * (double)t;
    }
    W[lane] = sd;
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): LDS writes visible wave-wide
  __builtin_amdgcn_wave_barrier();
  for (int iter = 0; iter < max_iter; iter++) {
    bool changed = false;
    for (int t = 1; t <= 2 * N - 3; t++) {
      const int j = t - lane;
      if (lane < j && j < N) changed |= jacobi_rotate<T, M, N, false>(At, W, nullptr, lane, j);
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
    }
    if (__ballot(changed) == 0) break;
  }
  if (lane == 0) jacobi_tail<T, M, N, N, false, false, true>(At, W, W, nullptr);
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
}

// _SVDcompute, m >= n, of a row-major M x N matrix A: left singular vectors as rows Ut (N x M), w, Vt.
template <class T, int M, int N, bool kV, bool kSmall>
CVSVD_HD void svd_rows(const T* A, T* Ut, double* w, T* Vt) {
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int k = 0; k < M; k++) Ut[i * M + k] = A[k * N + i];
  jacobi_svd<T, M, N, N, kV, kSmall>(Ut, w, Vt);
}

// SVBkSbImpl_<double> (kInv: b = identity, i.e. the inverse)
template <int M, int N, bool kInv>
CVSVD_HD void svd_backsubst(const double* Ut, const double* w, const double* Vt, const double* b, double* x) {
  constexpr int nb = kInv ? M : 1;
#pragma unroll
  for (int i = 0; i < N * nb; i++) x[i] = 0;
  double threshold = 0;
#pragma unroll
  for (int i = 0; i < N; i++) threshold += w[i];
  threshold *= DBL_EPSILON * 2;
#pragma unroll
  for (int i = 0; i < N; i++) {
    double wi = w[i];
    if (__builtin_fabs(wi) <= threshold) continue;
    wi = 1 / wi;
    const double* u = Ut + i * M;
    const double* v = Vt + i * N;
    if (!kInv) {
      double s = 0;
#pragma unroll
      for (int j = 0; j < M; j++) s += u[j] * b[j];
      s *= wi;
#pragma unroll
      for (int j = 0; j < N; j++) x[j] = x[j] + s * v[j];
    } else {
      double buffer[nb];
#pragma unroll
      for (int j = 0; j < nb; j++) buffer[j] = u[j] * wi;
#pragma unroll
      for (int j = 0; j < N; j++)
#pragma unroll
        for (int k = 0; k < nb; k++) x[j * nb + k] += buffer[k] * v[j];
    }
  }
}

#undef CVSVD_HD

}  // namespace cvsvd
}  // namespace orbx

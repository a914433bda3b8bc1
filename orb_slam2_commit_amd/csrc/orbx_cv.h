// orbx_cv.h -- OpenCV 3.2's arithmetic on 3x3 / 3x1 CV_32F Mats (modules/core/src/matmul.cpp: cv::gemm,
// GEMMSingleMul, dotProd_; lapack.cpp: det3, Mat::inv; convert.cpp: convertTo; stat.cpp: cv::norm),
// restated once for every unit that writes the reference's `R*X + t`, `-R.t()*t`, `K.inv()`, `x / norm(x)`:
// projection.hip, track.hip, triangulation.hip, sim3.hip, initializer.hip, newpoints.hip.  Float and
// double exactly where the library uses them, every sum in the library's order, -ffp-contract=off:
// nothing here may be re-associated.  __host__ __device__: the host builds of the Initializer and of
// CreateNewMapPoints run the same text.
//
// A matrix is a pointer and a compile-time row stride RS: 3 for a packed 3x3, 4 for the rotation block
// of a row-major 3x4 / 4x4 pose.  A 3x1 operand or result is three consecutive floats.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

namespace orbx {
namespace cvmat {

#define CVMAT_HD __host__ __device__ __forceinline__

// cv::gemm without a C, on the small-matrix path: OpenCV adds its zero C (`+ 0.0`, kPlusZero, which
// turns a -0 product into +0) -- or the site wrote the bare product, which keeps -0.  The two differ
// exactly at t0*alpha == -0 (known divergences).
enum NoC { kPlusZero, kBare };

// cv::gemm's small-matrix path (matmul.cpp: flags == 0, 2 <= len <= 4), 3x3 by 3x1: the dot product
// in float, left to right, then (float)(t0*alpha + c*beta) in double, beta = 1 -- with alpha = 1 a
// correctly rounded float add of c.  CS: the stride of c (4: the translation column of a pose).
// t0*1.0 and c*1.0 are exact, so a site that wrote (double)t0 + (double)c has these bits.
template <int RS, int CS = 1>
CVMAT_HD void gemm31_add(const float* A, const float* x, double alpha, const float* c, float* d) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float t0 = A[RS * i] * x[0] + A[RS * i + 1] * x[1] + A[RS * i + 2] * x[2];
    d[i] = (float)((double)t0 * alpha + (double)c[CS * i] * 1.0);
  }
}
// ... without a C
template <int RS, NoC kNoC = kPlusZero>
CVMAT_HD void gemm31(const float* A, const float* x, double alpha, float* d) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float t0 = A[RS * i] * x[0] + A[RS * i + 1] * x[1] + A[RS * i + 2] * x[2];
    d[i] = kNoC == kPlusZero ? (float)((double)t0 * alpha + 0.0) : (float)((double)t0 * alpha);
  }
}
// `R*X + t` of a pose T (row stride 4): cv::gemm(R, X, 1, t, 1)
CVMAT_HD void pose_apply(const float* T, const float* X, float* out) { gemm31_add<4, 4>(T, X, 1.0, T + 3, out); }

// ... 3x3 by 3x3, no C (+ 0.0).  A, B and D share the row stride.  With alpha = 1 the result is
// t0 + 0.0f in float: both turn -0 into +0 and are otherwise exact.
template <int RS>
CVMAT_HD void gemm33(const float* A, const float* B, double alpha, float* D) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const float t0 = A[RS * i] * B[j] + A[RS * i + 1] * B[RS + j] + A[RS * i + 2] * B[2 * RS + j];
      D[RS * i + j] = (float)((double)t0 * alpha + 0.0);
    }
}

// A * B.t() (a transpose flag leaves the small path): GEMMSingleMul<float,double>, the products summed
// in double from 0 in order, (float)(sum*alpha)
template <int RS>
CVMAT_HD void gemm33_bt(const float* A, const float* B, double alpha, float* D) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < 3; k++) s += (double)A[RS * i + k] * (double)B[RS * j + k];
      D[RS * i + j] = (float)(s * alpha);
    }
}
// A.t() * b (GEMM_1_T): the same path.  kFromZero = false starts the sum at the first product, which
// differs from 0 + the first product exactly when all three products are -0 (known
// divergences).  sum * -1.0 is -sum: an exact change of sign.
template <int RS, bool kFromZero>
CVMAT_HD void gemm31_at(const float* A, const float* b, double alpha, float* d) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    double s = (double)A[c] * (double)b[0];
    if (kFromZero) s = 0.0 + s;
    s = s + (double)A[RS + c] * (double)b[1];
    s = s + (double)A[2 * RS + c] * (double)b[2];
    d[c] = (float)(s * alpha);
  }
}

// det3 (lapack.cpp) of a 3x3 CV_32F, in double
template <int RS>
CVMAT_HD double det3(const float* m) {
  return m[0] * ((double)m[RS + 1] * m[2 * RS + 2] - (double)m[RS + 2] * m[2 * RS + 1]) -
         m[1] * ((double)m[RS] * m[2 * RS + 2] - (double)m[RS + 2] * m[2 * RS]) +
         m[2] * ((double)m[RS] * m[2 * RS + 1] - (double)m[RS + 1] * m[2 * RS]);
}

// Mat::inv() (DECOMP_LU) of a 3x3 CV_32F: the n == 3 special case; det == 0 gives zeros
template <int RS>
CVMAT_HD void inv3(const float* S, float* D) {
  double d = det3<RS>(S);
  if (d != 0.) {
    d = 1. / d;
    D[0] = (float)(((double)S[RS + 1] * S[2 * RS + 2] - (double)S[RS + 2] * S[2 * RS + 1]) * d);
    D[1] = (float)(((double)S[2] * S[2 * RS + 1] - (double)S[1] * S[2 * RS + 2]) * d);
    D[2] = (float)(((double)S[1] * S[RS + 2] - (double)S[2] * S[RS + 1]) * d);
    D[RS] = (float)(((double)S[RS + 2] * S[2 * RS] - (double)S[RS] * S[2 * RS + 2]) * d);
    D[RS + 1] = (float)(((double)S[0] * S[2 * RS + 2] - (double)S[2] * S[2 * RS]) * d);
    D[RS + 2] = (float)(((double)S[2] * S[RS] - (double)S[0] * S[RS + 2]) * d);
    D[2 * RS] = (float)(((double)S[RS] * S[2 * RS + 1] - (double)S[RS + 1] * S[2 * RS]) * d);
    D[2 * RS + 1] = (float)(((double)S[1] * S[2 * RS] - (double)S[0] * S[2 * RS + 1]) * d);
    D[2 * RS + 2] = (float)(((double)S[0] * S[RS + 1] - (double)S[1] * S[RS]) * d);
  } else {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) D[RS * r + c] = 0.f;
  }
}

// convertTo(alpha): x*(float)alpha + 0.0f, a copy when |alpha - 1| < DBL_EPSILON.  kCopyAtOne = false
// is a site that always multiplies: at such an alpha it differs for x == -0, which the product
// + 0.0f turns into +0 (known divergences).
template <bool kCopyAtOne = true>
CVMAT_HD float scale(float x, double alpha) {
  return kCopyAtOne && __builtin_fabs(alpha - 1) < DBL_EPSILON ? x : x * (float)alpha + 0.0f;
}

// Mat::dot of N floats (dotProd_): double products, summed four at a time and then the tail one by one,
// so N = 3 is a plain running sum and N = 9 is two sums of four and one product
template <int N>
CVMAT_HD double dot(const float* a, const float* b) {
  double s = 0;
  int i = 0;
#pragma unroll
  for (; i <= N - 4; i += 4)
    s += (double)a[i] * b[i] + (double)a[i + 1] * b[i + 1] + (double)a[i + 2] * b[i + 2] + (double)a[i + 3] * b[i + 3];
#pragma unroll
  for (; i < N; i++) s += (double)a[i] * (double)b[i];
  return s;
}

// cv::norm(NORM_L2) of 3 floats: the squares summed in double from 0 in order (a square is never -0,
// so starting at the first square gives the same bits), then the square root
CVMAT_HD double norm3(const float* v) {
  double s = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
  return __builtin_sqrt(s);
}

}  // namespace cvmat
}  // namespace orbx

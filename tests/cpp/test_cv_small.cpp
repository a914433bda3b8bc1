// test_cv_small.cpp -- orbx_cv.h and orbx_match.h on the host, under the address and
// undefined-behaviour sanitizers (tests/test_cv_small.py builds and runs it; no GPU call).
//   (no argument)  every cvmat routine at row strides 3 and 4 against plain loops in OpenCV's source
//                  order, bit for bit, on random inputs and on the inputs where the units' former
//                  copies could have differed; prints "cv small ok"
//   maxima         reads histograms (30 counts a line) from stdin, prints three_maxima's indices
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbx_cv.h"
#include "orbx_match.h"

using namespace orbx;
using namespace orbx::cvmat;

static int g_fail = 0;
static uint32_t bits(float x) {
  uint32_t b;
  std::memcpy(&b, &x, 4);
  return b;
}
static uint64_t bits(double x) {
  uint64_t b;
  std::memcpy(&b, &x, 8);
  return b;
}
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                               \
    }                                                         \
  } while (0)
static void same(const char* what, int rs, const float* got, const float* want, int n) {
  for (int k = 0; k < n; k++)
    if (bits(got[k]) != bits(want[k])) {
      std::printf("FAIL %s (stride %d) [%d]: %a (%08x) != %a (%08x)\n", what, rs, k, got[k], bits(got[k]), want[k],
                  bits(want[k]));
      g_fail++;
    }
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static float rnd() {  // [-2, 2), 16 random bits
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (float)((int)((g_rng >> 40) & 0xFFFF) - 32768) / 16384.f;
}

// ---- plain loops in OpenCV 3.2's order (run-time steps, as the library has them)
// matmul.cpp, cv::gemm's small-matrix path at len == 3: d = (float)(t0*alpha + c*beta), beta = 1
static void ref_gemm_small(const float* a, int a_step, const float* b, int b_step, int d_cols, double alpha,
                           const float* c, int c_step, bool plus_zero, float* d, int d_step) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < d_cols; j++) {
      const float t0 = a[i * a_step] * b[j] + a[i * a_step + 1] * b[b_step + j] + a[i * a_step + 2] * b[2 * b_step + j];
      if (c)
        d[i * d_step + j] = (float)(t0 * alpha + c[i * c_step + j] * 1.0);
      else if (plus_zero)
        d[i * d_step + j] = (float)(t0 * alpha + 0.0);
      else
        d[i * d_step + j] = (float)(t0 * alpha);
    }
}
// GEMMSingleMul<float,double>: element (i, j) of op(A) * op(B) with the elements' steps given
static float ref_single_mul(const float* a, int a_k, const float* b, int b_k, double alpha, bool from_zero) {
  double s = 0;
  for (int k = 0; k < 3; k++) {
    const double p = (double)a[k * a_k] * (double)b[k * b_k];
    s = (k == 0 && !from_zero) ? p : s + p;
  }
  return (float)(s * alpha);
}
#define Sf(y, x) S[(y) * rs + (x)]
static double ref_det3(const float* S, int rs) {
  return Sf(0, 0) * ((double)Sf(1, 1) * Sf(2, 2) - (double)Sf(1, 2) * Sf(2, 1)) -
         Sf(0, 1) * ((double)Sf(1, 0) * Sf(2, 2) - (double)Sf(1, 2) * Sf(2, 0)) +
         Sf(0, 2) * ((double)Sf(1, 0) * Sf(2, 1) - (double)Sf(1, 1) * Sf(2, 0));
}
static void ref_inv3(const float* S, int rs, float* D) {
  double d = ref_det3(S, rs);
  double t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (d != 0.) {
    d = 1. / d;
    t[0] = (((double)Sf(1, 1) * Sf(2, 2) - (double)Sf(1, 2) * Sf(2, 1)) * d);
    t[1] = (((double)Sf(0, 2) * Sf(2, 1) - (double)Sf(0, 1) * Sf(2, 2)) * d);
    t[2] = (((double)Sf(0, 1) * Sf(1, 2) - (double)Sf(0, 2) * Sf(1, 1)) * d);
    t[3] = (((double)Sf(1, 2) * Sf(2, 0) - (double)Sf(1, 0) * Sf(2, 2)) * d);
    t[4] = (((double)Sf(0, 0) * Sf(2, 2) - (double)Sf(0, 2) * Sf(2, 0)) * d);
    t[5] = (((double)Sf(0, 2) * Sf(1, 0) - (double)Sf(0, 0) * Sf(1, 2)) * d);
    t[6] = (((double)Sf(1, 0) * Sf(2, 1) - (double)Sf(1, 1) * Sf(2, 0)) * d);
    t[7] = (((double)Sf(0, 1) * Sf(2, 0) - (double)Sf(0, 0) * Sf(2, 1)) * d);
    t[8] = (((double)Sf(0, 0) * Sf(1, 1) - (double)Sf(0, 1) * Sf(1, 0)) * d);
  }
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) D[r * rs + c] = (float)t[3 * r + c];
}
#undef Sf
// dotProd_: four at a time, then the tail
static double ref_dot(const float* a, const float* b, int len) {
  double result = 0;
  int i = 0;
  for (; i <= len - 4; i += 4)
    result += (double)a[i] * b[i] + (double)a[i + 1] * b[i + 1] + (double)a[i + 2] * b[i + 2] + (double)a[i + 3] * b[i + 3];
  for (; i < len; i++) result += (double)a[i] * b[i];
  return result;
}
static double ref_norm3(const float* v) {
  double s = 0;
  for (int k = 0; k < 3; k++) s += (double)v[k] * v[k];
  return std::sqrt(s);
}
static float ref_scale(float x, double alpha, bool copy_at_one) {
  if (copy_at_one && std::fabs(alpha - 1) < DBL_EPSILON) return x;
  return x * (float)alpha + 0.0f;
}

// a packed 3x3 laid out at row stride RS in exactly 2 * RS + 3 floats (a read past a row's third
// element of the last row is out of bounds; the padding between rows is NaN)
template <int RS>
static std::vector<float> lay(const float* m) {
  std::vector<float> v(2 * RS + 3, std::nanf(""));
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) v[RS * r + c] = m[3 * r + c];
  return v;
}

template <int RS>
static void check_matrices(const float* A3, const float* B3, const float* x, const float* c) {
  const std::vector<float> A = lay<RS>(A3), B = lay<RS>(B3);
  const double alphas[] = {1.0, -1.0, 0.75, -2.5};
  for (double alpha : alphas) {
    float got[3], want[3];
    gemm31<RS, kPlusZero>(A.data(), x, alpha, got);
    ref_gemm_small(A.data(), RS, x, 1, 1, alpha, nullptr, 0, true, want, 1);
    same("gemm31 + 0.0", RS, got, want, 3);
    gemm31<RS, kBare>(A.data(), x, alpha, got);
    ref_gemm_small(A.data(), RS, x, 1, 1, alpha, nullptr, 0, false, want, 1);
    same("gemm31 bare", RS, got, want, 3);
    gemm31_add<RS, 1>(A.data(), x, alpha, c, got);
    ref_gemm_small(A.data(), RS, x, 1, 1, alpha, c, 1, true, want, 1);
    same("gemm31_add", RS, got, want, 3);
    // the addend at the stride of a pose's translation column
    const float c4[9] = {c[0], NAN, NAN, NAN, c[1], NAN, NAN, NAN, c[2]};
    gemm31_add<RS, 4>(A.data(), x, alpha, c4, got);
    same("gemm31_add, addend stride 4", RS, got, want, 3);

    std::vector<float> D(2 * RS + 3, 7.f), Dw(2 * RS + 3, 7.f);
    gemm33<RS>(A.data(), B.data(), alpha, D.data());
    ref_gemm_small(A.data(), RS, B.data(), RS, 3, alpha, nullptr, 0, true, Dw.data(), RS);
    same("gemm33", RS, D.data(), Dw.data(), 2 * RS + 3);
    gemm33_bt<RS>(A.data(), B.data(), alpha, D.data());
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) Dw[RS * i + j] = ref_single_mul(&A[RS * i], 1, &B[RS * j], 1, alpha, true);
    same("gemm33_bt", RS, D.data(), Dw.data(), 2 * RS + 3);
    for (int j = 0; j < 3; j++) want[j] = ref_single_mul(&A[j], RS, x, 1, alpha, true);
    gemm31_at<RS, true>(A.data(), x, alpha, got);
    same("gemm31_at from zero", RS, got, want, 3);
    for (int j = 0; j < 3; j++) want[j] = ref_single_mul(&A[j], RS, x, 1, alpha, false);
    gemm31_at<RS, false>(A.data(), x, alpha, got);
    same("gemm31_at from the first product", RS, got, want, 3);
  }
  CHECK(bits(det3<RS>(A.data())) == bits(ref_det3(A.data(), RS)));
  std::vector<float> D(2 * RS + 3, 7.f), Dw(2 * RS + 3, 7.f);
  inv3<RS>(A.data(), D.data());
  ref_inv3(A.data(), RS, Dw.data());
  same("inv3", RS, D.data(), Dw.data(), 2 * RS + 3);
}

static void check_pose_apply(const float* A3, const float* x, const float* c) {
  float T[12], got[3], want[3];
  for (int r = 0; r < 3; r++) {
    for (int k = 0; k < 3; k++) T[4 * r + k] = A3[3 * r + k];
    T[4 * r + 3] = c[r];
  }
  pose_apply(T, x, got);
  ref_gemm_small(T, 4, x, 1, 1, 1.0, T + 3, 4, true, want, 1);
  same("pose_apply", 4, got, want, 3);
  for (int r = 0; r < 3; r++) {  // the units' former spelling: a float add of t, correctly rounded
    const float t0 = T[4 * r] * x[0] + T[4 * r + 1] * x[1] + T[4 * r + 2] * x[2];
    want[r] = (float)((double)t0 + (double)T[4 * r + 3]);
  }
  same("pose_apply vs t0 + t", 4, got, want, 3);
}

static int self_check() {
  const float pz = 0.0f, nz = -0.0f;
  // random matrices
  for (int it = 0; it < 200; it++) {
    float A[9], B[9], x[3], c[3];
    for (float& v : A) v = rnd();
    for (float& v : B) v = rnd();
    for (float& v : x) v = rnd();
    for (float& v : c) v = rnd();
    check_matrices<3>(A, B, x, c);
    check_matrices<4>(A, B, x, c);
    check_pose_apply(A, x, c);
    float a9[9], b9[9];
    for (float& v : a9) v = rnd() * 1e3f;
    for (float& v : b9) v = rnd() * 1e-3f;
    CHECK(bits(dot<3>(a9, b9)) == bits(ref_dot(a9, b9, 3)));
    CHECK(bits(dot<9>(a9, b9)) == bits(ref_dot(a9, b9, 9)));
    CHECK(bits(norm3(a9)) == bits(ref_norm3(a9)));
  }
  // dot products that are exactly +0 and exactly -0, alpha = 1 and -1 (in check_matrices), addends of
  // either zero and a number
  const float ones[3] = {1.f, 1.f, 1.f};
  const float Az[2][9] = {{pz, pz, pz, pz, pz, pz, pz, pz, pz}, {nz, nz, nz, nz, nz, nz, nz, nz, nz}};
  const float cs[3][3] = {{pz, pz, pz}, {nz, nz, nz}, {1.5f, nz, pz}};
  for (const auto& A : Az)
    for (const auto& c : cs) {
      check_matrices<3>(A, A, ones, c);
      check_matrices<4>(A, A, ones, c);
      check_matrices<3>(A, Az[1], ones, c);
      check_pose_apply(A, ones, c);
    }
  {  // what the two no-C forms and the two starts of a double sum give at a zero, spelled out
    float d[3];
    gemm31<3, kPlusZero>(Az[0], ones, -1.0, d);  // t0 = +0, t0 * -1 = -0, + 0.0 = +0
    CHECK(bits(d[0]) == bits(pz));
    gemm31<3, kBare>(Az[0], ones, -1.0, d);
    CHECK(bits(d[0]) == bits(nz));
    gemm31<3, kPlusZero>(Az[1], ones, 1.0, d);  // t0 = -0
    CHECK(bits(d[0]) == bits(pz));
    gemm31<3, kBare>(Az[1], ones, 1.0, d);
    CHECK(bits(d[0]) == bits(nz));
    gemm31_at<3, true>(Az[1], ones, -1.0, d);  // 0 + -0 + -0 + -0 = +0
    CHECK(bits(d[0]) == bits(nz));
    gemm31_at<3, false>(Az[1], ones, -1.0, d);  // -0 + -0 + -0 = -0
    CHECK(bits(d[0]) == bits(pz));
  }
  {  // a singular matrix: zeros; an intrinsic matrix
    const float S[9] = {1.f, 2.f, 3.f, 2.f, 4.f, 6.f, -1.f, 0.5f, 7.f}, zero[3] = {0.f, 0.f, 0.f};
    check_matrices<3>(S, S, ones, zero);
    check_matrices<4>(S, S, ones, zero);
    float D[9];
    inv3<3>(S, D);
    for (float v : D) CHECK(bits(v) == bits(pz));
    const float K[9] = {718.856f, 0.f, 607.1928f, 0.f, 718.856f, 185.2157f, 0.f, 0.f, 1.f};
    check_matrices<3>(K, S, ones, zero);
    check_matrices<4>(K, S, ones, zero);
  }
  {  // convertTo: alpha within and just outside DBL_EPSILON of 1
    const double alphas[] = {1.0, 1.0 + DBL_EPSILON / 2, 1.0 - DBL_EPSILON / 2, 1.0 + DBL_EPSILON, 1.0 - DBL_EPSILON,
                             1.0 + 2 * DBL_EPSILON, 0.5, -1.0, 1.0 / 3};
    const float xs[] = {nz, pz, 3.7f, -1e-30f, 1e30f};
    for (double a : alphas)
      for (float x : xs) {
        CHECK(bits(scale(x, a)) == bits(ref_scale(x, a, true)));
        CHECK(bits(scale<false>(x, a)) == bits(ref_scale(x, a, false)));
      }
    CHECK(bits(scale(nz, 1.0)) == bits(nz) && bits(scale(nz, 1.0 + DBL_EPSILON / 2)) == bits(nz));  // copies
    CHECK(bits(scale(nz, 1.0 + DBL_EPSILON)) == bits(pz));                                           // -0 * 1.0f + 0.0f
    CHECK(bits(scale<false>(nz, 1.0)) == bits(pz));
  }
  // the rotation bin: the wrap at a negative difference, the half-way cases away from zero, bin 30
  CHECK(rot_bin(10.f, 10.f) == 0 && rot_bin(0.f, 14.9f) == 12 && rot_bin(45.f, 0.f) == 2 && rot_bin(44.9f, 0.f) == 1);
  CHECK(rot_bin(359.f, 0.f) == 12 && rot_bin(0.f, 1.f) == 12 && rot_bin(900.f, 0.f) == 0 && rot_bin(885.f, 0.f) == 0);
  if (g_fail) return 1;
  std::printf("cv small ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "maxima") == 0) {
    int h[30], sel[3];
    for (;;) {
      for (int& v : h)
        if (std::scanf("%d", &v) != 1) return 0;
      three_maxima(h, sel);
      std::printf("%d %d %d\n", sel[0], sel[1], sel[2]);
    }
  }
  return self_check();
}

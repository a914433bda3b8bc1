// test_initializer.cpp -- driver for the shim's ORB_SLAM2::Initializer (shim/include/Initializer.h),
// used by tests/test_initializer_shim.py.
//
//   test_initializer abi            signatures and members; without a device Initialize throws
//   test_initializer run IN OUT     Initializer(Frame, sigma, iterations) + Initialize per scene, in order,
//                                   all on the one process rand() stream (SeedRandOnce(0) on the first)
//   test_initializer chain IN OUT   ORBmatcher::SearchForInitialization -> Initializer::Initialize on a
//                                   two-view frame pair (Tracking::MonocularInitialization, :683-730)
// IN/OUT are little-endian binary files written/read by the Python test.  Exit status 0 = ok.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "Initializer.h"
#include "ORBmatcher.h"
#include "Objects.h"

using namespace ORB_SLAM2;

#define REQUIRE(c)                                                        \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "%s:%d: REQUIRE(%s)\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

struct Reader {
  FILE* f;
  explicit Reader(const char* p) : f(std::fopen(p, "rb")) { REQUIRE(f); }
  ~Reader() { std::fclose(f); }
  template <class T> T get() {
    T v;
    REQUIRE(std::fread(&v, sizeof(T), 1, f) == 1);
    return v;
  }
  template <class T> std::vector<T> vec(size_t n) {
    std::vector<T> v(n);
    if (n) REQUIRE(std::fread(v.data(), sizeof(T), n, f) == n);
    return v;
  }
};

struct Writer {
  FILE* f;
  explicit Writer(const char* p) : f(std::fopen(p, "wb")) { REQUIRE(f); }
  ~Writer() { std::fclose(f); }
  template <class T> void put(T v) { REQUIRE(std::fwrite(&v, sizeof(T), 1, f) == 1); }
  void mat(const cv::Mat& m, int rows, int cols) {
    REQUIRE(m.rows == rows && m.cols == cols && m.type() == CV_32F);
    for (int r = 0; r < rows; r++)
      for (int c = 0; c < cols; c++) put<float>(m.at<float>(r, c));
  }
};

static cv::Mat read_K(Reader& r) {
  cv::Mat K(3, 3, CV_32F);
  for (int i = 0; i < 9; i++) K.at<float>(i / 3, i % 3) = r.get<float>();
  return K;
}

static void set_keys(Frame& F, const std::vector<float>& xy) {
  const int n = (int)(xy.size() / 2);
  F.N = n;
  F.mvKeysUn.resize(n);
  for (int i = 0; i < n; i++) F.mvKeysUn[i] = cv::KeyPoint(xy[2 * i], xy[2 * i + 1], 31.f);
  F.mvKeys = F.mvKeysUn;
}

static int mode_abi() {
  // the reference's signatures (include/Initializer.h:36-45)
  static_assert(std::is_constructible<Initializer, const Frame&, float, int>::value, "ctor");
  static_assert(std::is_constructible<Initializer, const Frame&>::value, "ctor default sigma, iterations");
  bool (Initializer::*init)(const Frame&, const std::vector<int>&, cv::Mat&, cv::Mat&, std::vector<cv::Point3f>&,
                            std::vector<bool>&) = &Initializer::Initialize;
  REQUIRE(init);
  static_assert(sizeof(cv::Point3f) == 12, "cv::Point3f");
  // the constructor needs no device; Initialize exists only on one (no silent fallback), and fewer
  // than 8 matches are refused either way
  Frame F1, F2;
  F1.mK.create(3, 3, CV_32F);
  for (int i = 0; i < 9; i++) F1.mK.at<float>(i / 3, i % 3) = (i % 4) == 0 ? 1.f : 0.f;
  std::vector<float> xy;
  for (int i = 0; i < 12; i++) xy.push_back(10.f * i), xy.push_back(7.f * (i % 5));
  set_keys(F1, xy);
  set_keys(F2, xy);
  F2.mK = F1.mK.clone();
  Initializer I(F1, 1.0f, 5);
  std::vector<int> m(12, -1);
  for (int i = 0; i < 7; i++) m[i] = i;
  cv::Mat R, t;
  std::vector<cv::Point3f> P(3, cv::Point3f(1, 2, 3));
  std::vector<bool> vb(2, true);
  bool threw = false;
  try {
    (void)I.Initialize(F2, m, R, t, P, vb);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  REQUIRE(threw && R.empty() && t.empty() && P.size() == 3 && vb.size() == 2);
  std::printf("abi ok\n");
  return 0;
}

static void write_result(Writer& o, bool ok, const Initializer& I, const cv::Mat& R, const cv::Mat& t,
                         const std::vector<cv::Point3f>& P, const std::vector<bool>& vb) {
  const orbx_initializer_result& r = I.mResult;
  o.put<uint8_t>(ok);
  o.put<uint8_t>(R.empty());
  o.put<uint8_t>(t.empty());
  o.put<uint8_t>((uint8_t)r.degenerate);
  o.put<int32_t>(r.model);
  o.put<int32_t>(r.n_hyp);
  o.put<float>(r.SH);
  o.put<float>(r.SF);
  for (int k = 0; k < 8; k++) o.put<int32_t>(r.n_good[k]);
  for (int k = 0; k < 8; k++) o.put<float>(r.parallax[k]);
  o.put<int32_t>((int32_t)P.size());
  o.put<int32_t>((int32_t)vb.size());
  if (ok) {
    o.mat(R, 3, 3);
    o.mat(t, 3, 1);
  }
  for (const cv::Point3f& p : P) {
    o.put<float>(p.x);
    o.put<float>(p.y);
    o.put<float>(p.z);
  }
  for (size_t i = 0; i < vb.size(); i++) o.put<uint8_t>(vb[i]);
}

static int mode_run(const char* in, const char* out) {
  Reader r(in);
  Writer o(out);
  const int n_scenes = r.get<int32_t>();
  for (int s = 0; s < n_scenes; s++) {
    const int n1 = r.get<int32_t>(), n2 = r.get<int32_t>(), its = r.get<int32_t>();
    const float sigma = r.get<float>();
    Frame F1, F2;
    F1.mK = read_K(r);
    F2.mK = F1.mK.clone();
    set_keys(F1, r.vec<float>(2 * (size_t)n1));
    set_keys(F2, r.vec<float>(2 * (size_t)n2));
    const std::vector<int32_t> m32 = r.vec<int32_t>(n1);
    const std::vector<int> m(m32.begin(), m32.end());
    Initializer I(F1, sigma, its);
    // what a caller passes in: the outputs of an earlier attempt (untouched on false, R21 / t21 released)
    cv::Mat R(3, 3, CV_32F), t(3, 1, CV_32F);
    std::vector<cv::Point3f> P(2, cv::Point3f(9, 9, 9));
    std::vector<bool> vb(1, true);
    const bool ok = I.Initialize(F2, m, R, t, P, vb);
    write_result(o, ok, I, R, t, P, vb);
  }
  o.put<int32_t>(-1);
  std::printf("run ok: %d scenes\n", n_scenes);
  return 0;
}

// the frame layout of tests/test_shim.py's _frame_bytes (test_shim.cpp's read_frame), then K
static void read_frame(Reader& r, Frame& F) {
  const int n = r.get<int32_t>();
  F.N = n;
  F.mvKeysUn.resize(n);
  if (n) REQUIRE(std::fread(F.mvKeysUn.data(), 28, n, r.f) == (size_t)n);
  F.mvKeys = F.mvKeysUn;
  F.mDescriptors.create(n > 0 ? n : 1, 32, CV_8U);
  if (n) REQUIRE(std::fread(F.mDescriptors.data, 32, n, r.f) == (size_t)n);
  const int has_ur = r.get<int32_t>();
  F.mvuRight = has_ur ? r.vec<float>(n) : std::vector<float>(n, -1.f);
  (void)r.vec<int8_t>(n);
  F.mvpMapPoints.assign(n, nullptr);
  F.mvbOutlier.assign(n, false);
  Frame::mnMinX = r.get<float>();
  Frame::mnMaxX = r.get<float>();
  Frame::mnMinY = r.get<float>();
  Frame::mnMaxY = r.get<float>();
  Frame::mfGridElementWidthInv = r.get<float>();
  Frame::mfGridElementHeightInv = r.get<float>();
  F.mnScaleLevels = r.get<int32_t>();
  F.mvScaleFactors = r.vec<float>(F.mnScaleLevels);
  F.mvInvLevelSigma2 = r.vec<float>(F.mnScaleLevels);
  F.mvLevelSigma2.resize(F.mnScaleLevels);
  for (int l = 0; l < F.mnScaleLevels; l++) F.mvLevelSigma2[l] = F.mvScaleFactors[l] * F.mvScaleFactors[l];
  F.mfLogScaleFactor = r.get<float>();
  Frame::fx = r.get<float>();
  Frame::fy = r.get<float>();
  Frame::cx = r.get<float>();
  Frame::cy = r.get<float>();
  F.mbf = r.get<float>();
  F.mb = r.get<float>();
  cv::Mat T(4, 4, CV_32F);
  for (int i = 0; i < 16; i++) T.at<float>(i / 4, i % 4) = r.get<float>();
  F.SetPose(T);
}

static int mode_chain(const char* in, const char* out) {
  Reader r(in);
  const int window = r.get<int32_t>();
  const float nn = r.get<float>();
  const int check = r.get<int32_t>(), its = r.get<int32_t>();
  const float sigma = r.get<float>();
  Frame F1, F2;
  read_frame(r, F1);
  read_frame(r, F2);
  F1.mK = read_K(r);
  F2.mK = F1.mK.clone();
  std::vector<cv::Point2f> prev(F1.N);
  for (int i = 0; i < F1.N; i++) {
    const float x = r.get<float>();
    prev[i] = cv::Point2f(x, r.get<float>());
  }
  // Tracking::MonocularInitialization (src/Tracking.cc:683-730)
  Initializer I(F1, sigma, its);
  std::vector<int> m12;
  ORBmatcher matcher(nn, check != 0);
  const int nm = matcher.SearchForInitialization(F1, F2, prev, m12, window);
  cv::Mat R, t;
  std::vector<cv::Point3f> P;
  std::vector<bool> vb;
  const bool ok = I.Initialize(F2, m12, R, t, P, vb);
  Writer o(out);
  o.put<int32_t>(nm);
  for (int i = 0; i < F1.N; i++) o.put<int32_t>(m12[i]);
  write_result(o, ok, I, R, t, P, vb);
  o.put<int32_t>(-1);
  std::printf("chain ok: %d matches, Initialize %d\n", nm, (int)ok);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: test_initializer abi | run IN OUT | chain IN OUT\n");
    return 2;
  }
  try {
    const std::string m = argv[1];
    if (m == "abi") return mode_abi();
    if (m == "run" && argc == 4) return mode_run(argv[2], argv[3]);
    if (m == "chain" && argc == 4) return mode_chain(argv[2], argv[3]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "bad arguments\n");
  return 2;
}

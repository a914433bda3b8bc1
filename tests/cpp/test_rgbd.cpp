// test_rgbd.cpp -- driver of the shim's RGB-D front end for tests/test_rgbd_shim.py.
//
//   abi                 cv::Mat's 16-bit and multi-channel types, cv::cvtColor's argument checks; no device:
//                       the GPU members throw
//   rgbd    IN OUT      Frame's RGB-D constructor (the reference's signature on a grey image + CV_32F depth,
//                       or the raw-depth overload), then the monocular constructor on the same image;
//                       Frame::ComputeStereoFromRGBD as a member against the constructor's result
//   cvt     IN OUT      cv::cvtColor for CV_RGB2GRAY, CV_BGR2GRAY, CV_RGBA2GRAY, CV_BGRA2GRAY (one in place)
//
// IN / OUT are little-endian binary files laid out as the reads and writes below.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "ORBextractor.h"
#include "Objects.h"
#include "orbx.h"
#include "orbx_shim.h"

using namespace ORB_SLAM2;

#define REQUIRE(c)                                                    \
  do {                                                                \
    if (!(c)) {                                                       \
      std::fprintf(stderr, "REQUIRE failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                   \
    }                                                                 \
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
  void raw(const void* p, size_t n) {
    if (n) REQUIRE(std::fwrite(p, 1, n, f) == n);
  }
};

template <class E, class F> static bool throws(F f) {
  try {
    f();
  } catch (const E&) {
    return true;
  }
  return false;
}

static int mode_abi() {
  REQUIRE(CV_16U == 2 && CV_8UC3 == 16 && CV_8UC4 == 24 && CV_8UC1 == 0 && CV_32F == 5 && CV_64F == 6);
  REQUIRE(CV_BGR2GRAY == 6 && CV_RGB2GRAY == 7 && CV_BGRA2GRAY == 10 && CV_RGBA2GRAY == 11);
  REQUIRE(CV_16U == ORBX_DEPTH_U16 && CV_32F == ORBX_DEPTH_F32);
  cv::Mat d(3, 5, CV_16U), c3(3, 5, CV_8UC3), c4(3, 5, CV_8UC4), g(3, 5, CV_8U), f(3, 5, CV_32F);
  REQUIRE(d.channels() == 1 && d.depth() == CV_16U && d.elemSize() == 2 && d.step == 10 && d.isContinuous());
  REQUIRE(c3.channels() == 3 && c3.depth() == CV_8U && c3.elemSize() == 3 && c3.step == 15 && c3.type() == CV_8UC3);
  REQUIRE(c4.channels() == 4 && c4.elemSize() == 4 && c4.step == 20);
  REQUIRE(g.channels() == 1 && g.type() == CV_8UC1 && g.elemSize() == 1 && f.channels() == 1 && f.elemSize() == 4);
  d.at<uint16_t>(2, 4) = 65535;
  REQUIRE(d.clone().at<uint16_t>(2, 4) == 65535 && d.row(2).ptr<uint16_t>()[4] == 65535);
  std::memset(c3.data, 9, 45);
  REQUIRE(c3.clone().data[44] == 9);
  REQUIRE(throws<std::invalid_argument>([] { cv::Mat bad(2, 2, 1 /* CV_8S */); }));
  // cvtColor's argument checks come before any device call
  cv::Mat out;
  REQUIRE(throws<std::invalid_argument>([&] { cv::cvtColor(c3, out, CV_RGBA2GRAY); }));
  REQUIRE(throws<std::invalid_argument>([&] { cv::cvtColor(c4, out, CV_BGR2GRAY); }));
  REQUIRE(throws<std::invalid_argument>([&] { cv::cvtColor(g, out, CV_RGB2GRAY); }));
  REQUIRE(throws<std::invalid_argument>([&] { cv::cvtColor(c3, out, 40 /* CV_BGR2HSV */); }));
  if (orbx_device_count() <= 0) {
    REQUIRE(throws<std::runtime_error>([&] { cv::cvtColor(c3, out, CV_RGB2GRAY); }));
    REQUIRE(throws<std::runtime_error>([] { ORBextractor ex(500, 1.2f, 8, 20, 7); }));
    std::printf("abi ok (no device: GPU members throw)\n");
  } else {
    std::printf("abi ok (device present)\n");
  }
  return 0;
}

static void put_frame(Writer& o, const Frame& F) {
  o.put<int32_t>(F.N);
  REQUIRE((int)F.mvKeys.size() == F.N && (int)F.mvKeysUn.size() == F.N && (int)F.mvuRight.size() == F.N &&
          (int)F.mvDepth.size() == F.N && F.mDescriptors.rows == F.N && (int)F.mvpMapPoints.size() == F.N &&
          (int)F.mvbOutlier.size() == F.N);
  o.raw(F.mvKeys.data(), (size_t)F.N * 28);
  for (int i = 0; i < F.N; i++) o.raw(F.mDescriptors.ptr<uint8_t>(i), 32);
  o.raw(F.mvKeysUn.data(), (size_t)F.N * 28);
  o.raw(F.mvuRight.data(), (size_t)F.N * 4);
  o.raw(F.mvDepth.data(), (size_t)F.N * 4);
  o.put<float>(F.mb);
  o.put<float>(F.mfLogScaleFactor);
  o.put<int32_t>(F.mnScaleLevels);
  o.raw(F.mvScaleFactors.data(), F.mvScaleFactors.size() * 4);
  o.raw(F.mvInvLevelSigma2.data(), F.mvInvLevelSigma2.size() * 4);
}

static int mode_rgbd(const char* in, const char* out) {
  Reader r(in);
  const int w = r.get<int32_t>(), h = r.get<int32_t>(), nf = r.get<int32_t>(), ch = r.get<int32_t>();
  const int rgb = r.get<int32_t>(), dtype = r.get<int32_t>(), ref_ctor = r.get<int32_t>();
  const float factor = r.get<float>(), bf = r.get<float>();
  std::vector<float> Kv = r.vec<float>(9), dv = r.vec<float>(5);
  std::vector<uint8_t> img = r.vec<uint8_t>((size_t)w * h * ch);
  std::vector<uint8_t> dep = r.vec<uint8_t>((size_t)w * h * (dtype == CV_16U ? 2 : 4));
  cv::Mat K(3, 3, CV_32F), dist(5, 1, CV_32F);
  std::memcpy(K.data, Kv.data(), 36);
  std::memcpy(dist.data, dv.data(), 20);
  cv::Mat im(h, w, ch == 1 ? CV_8UC1 : ch == 3 ? CV_8UC3 : CV_8UC4, img.data());
  cv::Mat imDepth(h, w, dtype, dep.data());
  ORBextractor ex(nf, 1.2f, 8, 20, 7);
  const float thDepth = 40.f * bf / K.at<float>(0, 0);
  REQUIRE(Frame::mbInitialComputations);
  const long unsigned int id0 = Frame::nNextId;
  Frame F = ref_ctor ? Frame(im, imDepth, 1.5, &ex, nullptr, K, dist, bf, thDepth)
                     : Frame(im, imDepth, 1.5, &ex, nullptr, K, dist, bf, thDepth, factor, rgb != 0);
  REQUIRE(!Frame::mbInitialComputations && F.mnId == id0 && Frame::nNextId == id0 + 1 && F.mTimeStamp == 1.5);
  REQUIRE(F.mpORBextractorLeft == &ex && F.mpORBextractorRight == nullptr && F.mbf == bf && F.mThDepth == thDepth);
  for (int l = 0; l < 8; l++) REQUIRE(ex.mvImagePyramid[l].empty());
  Writer o(out);
  put_frame(o, F);
  const float statics[12] = {Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY, Frame::mfGridElementWidthInv,
                             Frame::mfGridElementHeightInv, Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx,
                             Frame::invfy};
  o.raw(statics, sizeof(statics));
  // the member on its own: the reference's loop over a CV_32F image the constructor saw unscaled
  if (dtype == CV_32F && (ref_ctor || factor == 1.0f)) {
    Frame G = F;
    G.mvuRight.assign(G.N, 7.f);
    G.mvDepth.assign(G.N, 7.f);
    G.ComputeStereoFromRGBD(imDepth);
    REQUIRE(std::memcmp(G.mvuRight.data(), F.mvuRight.data(), (size_t)F.N * 4) == 0);
    REQUIRE(std::memcmp(G.mvDepth.data(), F.mvDepth.data(), (size_t)F.N * 4) == 0);
  }
  // the monocular constructor on the grey image
  cv::Mat grey = im;
  if (ch > 1) cv::cvtColor(im, grey, ch == 3 ? (rgb ? CV_RGB2GRAY : CV_BGR2GRAY) : (rgb ? CV_RGBA2GRAY : CV_BGRA2GRAY));
  REQUIRE(grey.type() == CV_8UC1 && (ch == 1 || grey.data != im.data));
  Frame M(grey, 2.5, &ex, nullptr, K, dist, bf, thDepth);
  REQUIRE(M.mnId == id0 + 1 && M.mTimeStamp == 2.5 && M.N == F.N);
  for (int i = 0; i < M.N; i++) REQUIRE(M.mvuRight[i] == -1.0f && M.mvDepth[i] == -1.0f);
  put_frame(o, M);
  // an empty image: N = 0, nothing else touched (src/Frame.cc:147-148, 208-209)
  Frame E(cv::Mat(), cv::Mat(), 3.5, &ex, nullptr, K, dist, bf, thDepth, factor, true);
  REQUIRE(E.N == 0 && E.mvKeys.empty() && E.mvuRight.empty() && E.mnId == id0 + 2 && E.mnScaleLevels == 8);
  // a depth image of another size, or of a type the reference's constructor cannot index, is an error
  cv::Mat small(h - 1, w, dtype, dep.data());
  REQUIRE(throws<std::runtime_error>([&] { Frame X(im, small, 0.0, &ex, nullptr, K, dist, bf, thDepth, factor, true); }));
  if (dtype == CV_16U && ch == 1)
    REQUIRE(throws<std::invalid_argument>([&] { Frame X(im, imDepth, 0.0, &ex, nullptr, K, dist, bf, thDepth); }));
  std::printf("rgbd ok: N=%d\n", F.N);
  return 0;
}

static int mode_cvt(const char* in, const char* out) {
  Reader r(in);
  const int w = r.get<int32_t>(), h = r.get<int32_t>();
  std::vector<uint8_t> px4 = r.vec<uint8_t>((size_t)w * h * 4);
  cv::Mat c4(h, w, CV_8UC4, px4.data()), c3(h, w, CV_8UC3);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) std::memcpy(c3.ptr<uint8_t>(y) + 3 * x, c4.ptr<uint8_t>(y) + 4 * x, 3);
  Writer o(out);
  const int codes[4] = {CV_RGB2GRAY, CV_BGR2GRAY, CV_RGBA2GRAY, CV_BGRA2GRAY};
  for (int k = 0; k < 4; k++) {
    cv::Mat g;
    cv::cvtColor(k < 2 ? c3 : c4, g, codes[k]);
    REQUIRE(g.type() == CV_8UC1 && g.rows == h && g.cols == w && g.channels() == 1);
    for (int y = 0; y < h; y++) o.raw(g.ptr<uint8_t>(y), w);
  }
  // in place, as src/Tracking.cc:178 calls it: cvtColor(mImGray,mImGray,CV_RGB2GRAY); a Mat that shared
  // the colour data keeps it
  cv::Mat m = c3.clone(), keep = m;
  cv::cvtColor(m, m, CV_RGB2GRAY);
  REQUIRE(m.type() == CV_8UC1 && m.cols == w && keep.type() == CV_8UC3 && keep.data != m.data);
  REQUIRE(std::memcmp(keep.data, c3.data, (size_t)w * h * 3) == 0);
  for (int y = 0; y < h; y++) o.raw(m.ptr<uint8_t>(y), w);
  std::printf("cvt ok\n");
  return 0;
}

int main(int argc, char** argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "abi") return mode_abi();
    if (mode == "rgbd" && argc == 4) return mode_rgbd(argv[2], argv[3]);
    if (mode == "cvt" && argc == 4) return mode_cvt(argv[2], argv[3]);
    std::fprintf(stderr, "usage: test_rgbd abi | rgbd IN OUT | cvt IN OUT\n");
    return 2;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
}

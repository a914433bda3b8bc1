// test_globalba.cpp -- driver of tests/test_globalba_shim.py: builds a Map of KeyFrame / MapPoint objects
// with their observations from the file the Python side wrote and calls the shim's
// Optimizer::GlobalBundleAdjustemnt through the reference signature (src/Optimizer.cc:41), writing what
// the reference's caller sees afterwards: every keyframe's pose, mTcwGBA and mnBAGlobalForKF, every map
// point's position, mPosGBA and mnBAGlobalForKF.
//   test_globalba abi            the two signatures with the reference's defaults and the members the
//                                function writes; without a device the call throws
//   test_globalba run IN OUT     GlobalBundleAdjustemnt on the map of the file
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "Objects.h"
#include "Optimizer.h"

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

static cv::Mat pose_of(const float* T12) {
  cv::Mat T(4, 4, CV_32F);
  for (int i = 0; i < 12; i++) T.at<float>(i / 4, i % 4) = T12[i];
  for (int c = 0; c < 4; c++) T.at<float>(3, c) = c == 3 ? 1.f : 0.f;
  return T;
}

struct World {
  Map map;
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  std::vector<std::unique_ptr<MapPoint>> points;
  std::map<long unsigned int, KeyFrame*> byId;
  int nLoopKF = 0, nIterations = 5;
  bool bRobust = true;
};

// int32 nkf, npt, nLoopKF, nIterations, bRobust | float[8] mvInvLevelSigma2 | float[8] mvScaleFactors |
// per keyframe: int64 mnId, float[12] Tcw, int32 bad, float[5] fx fy cx cy mbf |
// per point: int64 mnId, float[3] pos, int32 bad, int32 nobs, nobs x (int32 keyframe id, float u v ur, int32 octave)
static void read_world(Reader& in, World& W) {
  const int32_t nkf = in.get<int32_t>(), npt = in.get<int32_t>();
  W.nLoopKF = in.get<int32_t>();
  W.nIterations = in.get<int32_t>();
  W.bRobust = in.get<int32_t>() != 0;
  const std::vector<float> inv = in.vec<float>(8), sf = in.vec<float>(8);
  for (int k = 0; k < nkf; k++) {
    std::unique_ptr<KeyFrame> kf(new KeyFrame());
    kf->mnId = (long unsigned int)in.get<int64_t>();
    const std::vector<float> T = in.vec<float>(12);
    kf->SetPose(pose_of(T.data()));
    kf->mbBad = in.get<int32_t>() != 0;
    const std::vector<float> K = in.vec<float>(5);
    kf->fx = K[0], kf->fy = K[1], kf->cx = K[2], kf->cy = K[3], kf->mbf = K[4];
    kf->mvInvLevelSigma2 = inv;
    kf->mvScaleFactors = sf;
    kf->mnScaleLevels = 8;
    W.byId[kf->mnId] = kf.get();
    W.map.mspKeyFrames.insert(kf.get());
    if (kf->mnId > W.map.mnMaxKFid) W.map.mnMaxKFid = kf->mnId;
    W.kfs.push_back(std::move(kf));
  }
  for (int j = 0; j < npt; j++) {
    const long unsigned int id = (long unsigned int)in.get<int64_t>();
    const std::vector<float> X = in.vec<float>(3);
    cv::Mat pos(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) pos.at<float>(k, 0) = X[k];
    std::unique_ptr<MapPoint> mp(new MapPoint(pos, nullptr, &W.map));
    mp->mnId = id;
    const bool bad = in.get<int32_t>() != 0;
    const int32_t nobs = in.get<int32_t>();
    for (int o = 0; o < nobs; o++) {
      KeyFrame* kf = W.byId.at((long unsigned int)in.get<int32_t>());
      const std::vector<float> uvr = in.vec<float>(3);
      const int32_t octave = in.get<int32_t>();
      const size_t idx = kf->mvKeysUn.size();
      kf->mvKeysUn.push_back(cv::KeyPoint(uvr[0], uvr[1], 31.f, -1.f, 0.f, octave));
      kf->mvuRight.push_back(uvr[2]);
      kf->mvpMapPoints.push_back(mp.get());
      kf->N = (int)kf->mvKeysUn.size();
      mp->AddObservation(kf, idx);
      if (!mp->mpRefKF) mp->mpRefKF = kf;
    }
    mp->mbBad = bad;
    W.map.mspMapPoints.insert(mp.get());
    W.points.push_back(std::move(mp));
  }
}

static int mode_abi() {
  void (*g)(Map*, int, bool*, const unsigned long, const bool) = &Optimizer::GlobalBundleAdjustemnt;
  void (*b)(const std::vector<KeyFrame*>&, const std::vector<MapPoint*>&, int, bool*, const unsigned long, const bool) =
      &Optimizer::BundleAdjustment;
  REQUIRE(g && b);
  KeyFrame a, c;
  a.mnId = 0, c.mnId = 1;
  const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  a.SetPose(pose_of(I));
  c.SetPose(pose_of(I));
  REQUIRE(a.mTcwGBA.empty() && a.mnBAGlobalForKF == 0);
  Map map;
  map.mspKeyFrames = {&a, &c};
  map.mnMaxKFid = 1;
  cv::Mat pos(3, 1, CV_32F);
  for (int k = 0; k < 3; k++) pos.at<float>(k, 0) = 1.f + k;
  MapPoint mp(pos, nullptr, &map);
  map.mspMapPoints.insert(&mp);
  REQUIRE(mp.mPosGBA.empty() && mp.mnBAGlobalForKF == 0);
  // the reference's defaults: (pMap) alone is a call; it exists only on a device (no silent fallback)
  bool threw = false;
  try {
    Optimizer::GlobalBundleAdjustemnt(&map);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  // (on a device: the point has no edge, so it stays; the poses come back through the conversions)
  REQUIRE(threw || (mp.GetWorldPos().at<float>(0, 0) == 1.f && c.GetPose().at<float>(0, 0) == 1.f));
  std::printf("abi ok\n");
  return 0;
}

static int mode_run(const char* in_path, const char* out_path) {
  Reader in(in_path);
  World W;
  read_world(in, W);
  Optimizer::GlobalBundleAdjustemnt(&W.map, W.nIterations, nullptr, (unsigned long)W.nLoopKF, W.bRobust);
  FILE* f = std::fopen(out_path, "wb");
  REQUIRE(f);
  const auto put = [&](float v) { REQUIRE(std::fwrite(&v, 4, 1, f) == 1); };
  for (const auto& kf : W.kfs) {
    const cv::Mat T = kf->GetPose();
    for (int i = 0; i < 12; i++) put(T.at<float>(i / 4, i % 4));
    for (int i = 0; i < 12; i++) put(kf->mTcwGBA.empty() ? 0.f : kf->mTcwGBA.at<float>(i / 4, i % 4));
    put((float)kf->mnBAGlobalForKF);
  }
  for (const auto& mp : W.points) {
    const cv::Mat X = mp->GetWorldPos();
    for (int k = 0; k < 3; k++) put(X.at<float>(k, 0));
    for (int k = 0; k < 3; k++) put(mp->mPosGBA.empty() ? 0.f : mp->mPosGBA.at<float>(k, 0));
    put((float)mp->mnBAGlobalForKF);
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "abi") return mode_abi();
  if (argc == 4 && std::string(argv[1]) == "run") return mode_run(argv[2], argv[3]);
  std::fprintf(stderr, "usage: test_globalba abi | run IN OUT\n");
  return 2;
}

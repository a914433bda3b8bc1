// test_newpoints.cpp -- driver of tests/test_newpoints_shim.py: builds a Map of KeyFrame / MapPoint objects
// from the file the Python side wrote (the current keyframe, then its neighbours in covisibility order) and
// calls the shim's LocalMapping::CreateNewMapPoints() (src/LocalMapping.cc:281-558), writing what the
// reference's caller sees afterwards: mlpRecentAddedMapPoints in order with every point's position and
// observations, and each keyframe's mvpMapPoints.
//   test_newpoints abi                  the reference's members; without a device the call throws
//   test_newpoints run IN OUT           CreateNewMapPoints on the graph of the file
//   test_newpoints chain IN OUT         ... followed by Optimizer::LocalBundleAdjustment on the same graph
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "LocalMapping.h"
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

struct World {
  Map map;
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  std::vector<std::unique_ptr<MapPoint>> old_points;
  int monocular = 0, stop = 0;
  float scale_factor = 1.2f;
};

// int32 nkf, monocular, stop | float mfScaleFactor | per keyframe: int32 n, n_nodes, n_levels, float Tcw[16],
// float fx fy cx cy mb mbf, float sf[n_levels], sigma2[n_levels], n x (x, y, size, angle, response, int32 octave,
// int32 class_id) mvKeysUn, float mvKeys xy[2n], mvuRight[n], mvDepth[n], uint8 desc[32n], has_mp[n],
// float mp_pos[3n], uint32 node_id[n_nodes], int32 node_off[n_nodes + 1], int32 feat[node_off[n_nodes]]
static void read_world(Reader& in, World& W) {
  const int32_t nkf = in.get<int32_t>();
  W.monocular = in.get<int32_t>();
  W.stop = in.get<int32_t>();
  W.scale_factor = in.get<float>();
  for (int k = 0; k < nkf; k++) {
    std::unique_ptr<KeyFrame> kf(new KeyFrame());
    kf->mnId = (long unsigned int)((k + 1) % nkf);  // (the last neighbour is keyframe 0: LocalBA's fixed one)
    const int32_t n = in.get<int32_t>(), nn = in.get<int32_t>(), nl = in.get<int32_t>();
    const std::vector<float> T = in.vec<float>(16);
    cv::Mat Tcw(4, 4, CV_32F);
    for (int i = 0; i < 16; i++) Tcw.at<float>(i / 4, i % 4) = T[i];
    kf->SetPose(Tcw);
    const std::vector<float> K = in.vec<float>(6);
    kf->fx = K[0], kf->fy = K[1], kf->cx = K[2], kf->cy = K[3], kf->mb = K[4], kf->mbf = K[5];
    kf->invfx = 1.0f / kf->fx, kf->invfy = 1.0f / kf->fy;
    kf->mnScaleLevels = nl;
    kf->mfScaleFactor = W.scale_factor;
    kf->mvScaleFactors = in.vec<float>(nl);
    kf->mvLevelSigma2 = in.vec<float>(nl);
    kf->mvInvLevelSigma2.resize(nl);
    for (int l = 0; l < nl; l++) kf->mvInvLevelSigma2[l] = 1.0f / kf->mvLevelSigma2[l];
    kf->N = n;
    struct Kp {
      float x, y, size, angle, response;
      int32_t octave, class_id;
    };
    const std::vector<Kp> kps = in.vec<Kp>(n);
    const std::vector<float> xy = in.vec<float>(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
      kf->mvKeysUn.push_back(cv::KeyPoint(kps[i].x, kps[i].y, kps[i].size, kps[i].angle, kps[i].response, kps[i].octave));
      kf->mvKeys.push_back(cv::KeyPoint(xy[2 * i], xy[2 * i + 1], kps[i].size, kps[i].angle, kps[i].response, kps[i].octave));
    }
    kf->mvuRight = in.vec<float>(n);
    kf->mvDepth = in.vec<float>(n);
    const std::vector<uint8_t> desc = in.vec<uint8_t>(32 * (size_t)n);
    kf->mDescriptors = cv::Mat(n, 32, CV_8U);
    if (n) std::memcpy(kf->mDescriptors.data, desc.data(), desc.size());
    const std::vector<uint8_t> has = in.vec<uint8_t>(n);
    const std::vector<float> mp = in.vec<float>(3 * (size_t)n);
    kf->mvpMapPoints.assign(n, nullptr);
    for (int i = 0; i < n; i++)
      if (has[i]) {
        cv::Mat pos(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) pos.at<float>(c, 0) = mp[3 * i + c];
        std::unique_ptr<MapPoint> p(new MapPoint(pos, kf.get(), &W.map));
        p->AddObservation(kf.get(), i);
        kf->mvpMapPoints[i] = p.get();
        W.map.mspMapPoints.insert(p.get());
        W.old_points.push_back(std::move(p));
      }
    const std::vector<uint32_t> ids = in.vec<uint32_t>(nn);
    const std::vector<int32_t> off = in.vec<int32_t>(nn + 1);
    const std::vector<int32_t> feat = in.vec<int32_t>(nn ? off[nn] : 0);
    for (int j = 0; j < nn; j++)
      for (int q = off[j]; q < off[j + 1]; q++) kf->mFeatVec[ids[j]].push_back((unsigned int)feat[q]);
    W.map.mspKeyFrames.insert(kf.get());
    if (kf->mnId > W.map.mnMaxKFid) W.map.mnMaxKFid = kf->mnId;
    W.kfs.push_back(std::move(kf));
  }
  KeyFrame* cur = W.kfs[0].get();
  for (size_t k = 1; k < W.kfs.size(); k++) {  // covisibility: the file's order, weights descending
    cur->mvpOrderedConnectedKeyFrames.push_back(W.kfs[k].get());
    cur->mvOrderedWeights.push_back(1000 - (int)k);
    cur->mConnectedKeyFrameWeights[W.kfs[k].get()] = 1000 - (int)k;
    W.kfs[k]->mvpOrderedConnectedKeyFrames.push_back(cur);
    W.kfs[k]->mvOrderedWeights.push_back(1000 - (int)k);
    W.kfs[k]->mConnectedKeyFrameWeights[cur] = 1000 - (int)k;
  }
}

static int mode_abi() {
  // the reference's members (include/LocalMapping.h:44, :50, :89, :95) and what CreateNewMapPoints touches
  void (LocalMapping::*ins)(KeyFrame*) = &LocalMapping::InsertKeyFrame;
  bool (LocalMapping::*chk)() = &LocalMapping::CheckNewKeyFrames;
  void (LocalMapping::*cnmp)() = &LocalMapping::CreateNewMapPoints;
  REQUIRE(ins && chk && cnmp);
  Map map;
  LocalMapping lm(&map, 0.f);
  REQUIRE(!lm.mbMonocular && !lm.CheckNewKeyFrames() && lm.mlpRecentAddedMapPoints.empty() && !lm.mpCurrentKeyFrame);
  KeyFrame a;
  const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  cv::Mat T(4, 4, CV_32F);
  for (int i = 0; i < 16; i++) T.at<float>(i / 4, i % 4) = I[i];
  a.SetPose(T);
  a.mvScaleFactors = {1.f}, a.mvLevelSigma2 = {1.f};
  a.mnScaleLevels = 1;
  a.fx = a.fy = 500.f;
  lm.InsertKeyFrame(&a);
  REQUIRE(lm.CheckNewKeyFrames() && lm.mbAbortBA && lm.mlNewKeyFrames.front() == &a);
  lm.mpCurrentKeyFrame = &a;
  bool threw = false;
  try {
    lm.CreateNewMapPoints();  // no neighbour: nothing to make; it exists only on a device (no silent fallback)
  } catch (const std::runtime_error&) {
    threw = true;
  }
  REQUIRE(threw || (lm.mlpRecentAddedMapPoints.empty() && lm.mnNeighboursDone == 0));
  std::printf("abi ok\n");
  return 0;
}

static int mode_run(const char* in_path, const char* out_path, bool chain) {
  Reader in(in_path);
  World W;
  read_world(in, W);
  LocalMapping lm(&W.map, W.monocular ? 1.f : 0.f);
  lm.mpCurrentKeyFrame = W.kfs[0].get();
  KeyFrame queued;
  if (W.stop) lm.InsertKeyFrame(&queued);
  lm.CreateNewMapPoints();
  FILE* f = std::fopen(out_path, "wb");
  REQUIRE(f);
  const auto puti = [&](int32_t v) { REQUIRE(std::fwrite(&v, 4, 1, f) == 1); };
  const auto putf = [&](float v) { REQUIRE(std::fwrite(&v, 4, 1, f) == 1); };
  std::map<KeyFrame*, int> kf_index;
  for (size_t k = 0; k < W.kfs.size(); k++) kf_index[W.kfs[k].get()] = (int)k;
  std::map<MapPoint*, int> recent;
  puti((int32_t)lm.mlpRecentAddedMapPoints.size());
  puti(lm.mnNeighboursDone);
  for (MapPoint* p : lm.mlpRecentAddedMapPoints) {
    const int at = (int)recent.size();
    recent[p] = at;
    REQUIRE(W.map.mspMapPoints.count(p) == 1 && p->GetReferenceKeyFrame() == W.kfs[0].get());
    REQUIRE(!p->GetDescriptor().empty() && p->GetMaxDistanceInvariance() > 0.f);
    const cv::Mat X = p->GetWorldPos();
    for (int c = 0; c < 3; c++) putf(X.at<float>(c, 0));
    std::vector<std::pair<int, int>> obs;
    for (const auto& o : p->mObservations) obs.push_back({kf_index.at(o.first), (int)o.second});
    std::sort(obs.begin(), obs.end());
    puti((int32_t)obs.size());
    for (const auto& o : obs) {
      puti(o.first);
      puti(o.second);
    }
  }
  for (const auto& kf : W.kfs) {
    puti(kf->N);
    for (int i = 0; i < kf->N; i++) {
      MapPoint* p = kf->GetMapPoint(i);
      puti(!p ? -1 : (recent.count(p) ? recent[p] : -2));
    }
  }
  if (chain) {  // LocalMapping::Run's next numeric step on the same graph (src/LocalMapping.cc:101-102)
    bool stop = false;
    Optimizer::LocalBundleAdjustment(W.kfs[0].get(), &stop, &W.map);
    for (MapPoint* p : lm.mlpRecentAddedMapPoints) {
      const cv::Mat X = p->GetWorldPos();
      for (int c = 0; c < 3; c++) putf(X.at<float>(c, 0));
      puti(p->isBad() ? 1 : 0);
    }
    const cv::Mat T = W.kfs[0]->GetPose();
    for (int i = 0; i < 12; i++) putf(T.at<float>(i / 4, i % 4));
  }
  std::fclose(f);
  for (MapPoint* p : lm.mlpRecentAddedMapPoints) delete p;
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "abi") return mode_abi();
  if (argc == 4 && std::string(argv[1]) == "run") return mode_run(argv[2], argv[3], false);
  if (argc == 4 && std::string(argv[1]) == "chain") return mode_run(argv[2], argv[3], true);
  std::fprintf(stderr, "usage: test_newpoints abi | run IN OUT | chain IN OUT\n");
  return 2;
}

// test_essgraph.cpp -- driver of tests/test_essgraph_shim.py: builds a Map of KeyFrame / MapPoint objects
// from the file the Python side wrote and calls the shim's Optimizer::OptimizeEssentialGraph through the
// reference signature (src/Optimizer.cc:888), writing what the reference's caller sees afterwards: every
// keyframe's pose and every map point's position.
//   test_essgraph abi            the signature, the typedef and the members the function reads; without a
//                                device the call throws
//   test_essgraph run IN OUT     OptimizeEssentialGraph on the map of the file
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <set>
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

static g2o::Sim3 sim3_of(const std::vector<double>& v) {
  return g2o::Sim3(g2o::Quaterniond(v[3], v[0], v[1], v[2]), g2o::Vector3d{v[4], v[5], v[6]}, v[7]);
}

struct World {
  Map map;
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  std::vector<std::unique_ptr<MapPoint>> points;
  std::map<long unsigned int, KeyFrame*> byId;
  KeyFrame *pLoopKF = nullptr, *pCurKF = nullptr;
  LoopClosing::KeyFrameAndPose NonCorrectedSim3, CorrectedSim3;
  std::map<KeyFrame*, std::set<KeyFrame*>> LoopConnections;
  bool bFixScale = false;
};

static void read_world(Reader& in, World& W) {
  const int32_t nkf = in.get<int32_t>(), npt = in.get<int32_t>();
  const int32_t loopId = in.get<int32_t>(), curId = in.get<int32_t>();
  W.bFixScale = in.get<int32_t>() != 0;
  struct Links {
    int32_t parent;
    std::vector<int32_t> children, loops, cov;
  };
  std::vector<Links> links(nkf);
  for (int k = 0; k < nkf; k++) {
    std::unique_ptr<KeyFrame> kf(new KeyFrame());
    kf->mnId = (long unsigned int)in.get<int64_t>();
    const std::vector<float> T = in.vec<float>(12);
    kf->SetPose(pose_of(T.data()));
    kf->mbBad = in.get<int32_t>() != 0;
    links[k].parent = in.get<int32_t>();
    links[k].children = in.vec<int32_t>((size_t)in.get<int32_t>());
    links[k].loops = in.vec<int32_t>((size_t)in.get<int32_t>());
    links[k].cov = in.vec<int32_t>(2 * (size_t)in.get<int32_t>());
    W.byId[kf->mnId] = kf.get();
    W.map.mspKeyFrames.insert(kf.get());
    if (kf->mnId > W.map.mnMaxKFid) W.map.mnMaxKFid = kf->mnId;
    W.kfs.push_back(std::move(kf));
  }
  for (int k = 0; k < nkf; k++) {
    KeyFrame* kf = W.kfs[k].get();
    if (links[k].parent >= 0) kf->mpParent = W.byId.at(links[k].parent);
    for (int32_t c : links[k].children) kf->mspChildrens.insert(W.byId.at(c));
    for (int32_t l : links[k].loops) kf->mspLoopEdges.insert(W.byId.at(l));
    for (size_t j = 0; j + 1 < links[k].cov.size(); j += 2) {
      KeyFrame* o = W.byId.at(links[k].cov[j]);
      kf->mvpOrderedConnectedKeyFrames.push_back(o);
      kf->mvOrderedWeights.push_back(links[k].cov[j + 1]);
      kf->mConnectedKeyFrameWeights[o] = links[k].cov[j + 1];
    }
  }
  W.pLoopKF = W.byId.at(loopId);
  W.pCurKF = W.byId.at(curId);
  for (LoopClosing::KeyFrameAndPose* dst : {&W.NonCorrectedSim3, &W.CorrectedSim3}) {
    const int32_t m = in.get<int32_t>();
    for (int j = 0; j < m; j++) {
      const int32_t id = in.get<int32_t>();
      (*dst)[W.byId.at(id)] = sim3_of(in.vec<double>(8));
    }
  }
  const int32_t nconn = in.get<int32_t>();
  for (int j = 0; j < nconn; j++) {
    const int32_t id = in.get<int32_t>();
    const std::vector<int32_t> others = in.vec<int32_t>((size_t)in.get<int32_t>());
    for (int32_t o : others) W.LoopConnections[W.byId.at(id)].insert(W.byId.at(o));
  }
  for (int j = 0; j < npt; j++) {
    const std::vector<float> X = in.vec<float>(3);
    cv::Mat pos(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) pos.at<float>(k, 0) = X[k];
    const int32_t ref = in.get<int32_t>();
    std::unique_ptr<MapPoint> mp(new MapPoint(pos, W.byId.at(ref), &W.map));
    mp->mnCorrectedByKF = (long unsigned int)in.get<int64_t>();
    mp->mnCorrectedReference = (long unsigned int)in.get<int64_t>();
    mp->mbBad = in.get<int32_t>() != 0;
    W.map.mspMapPoints.insert(mp.get());
    W.points.push_back(std::move(mp));
  }
}

static int mode_abi() {
  void (*f)(Map*, KeyFrame*, KeyFrame*, const LoopClosing::KeyFrameAndPose&, const LoopClosing::KeyFrameAndPose&,
            const std::map<KeyFrame*, std::set<KeyFrame*>>&, const bool&) = &Optimizer::OptimizeEssentialGraph;
  REQUIRE(f);
  // the members the function reads, with the reference's semantics
  KeyFrame a, b, c;
  a.mnId = 0, b.mnId = 1, c.mnId = 2;
  const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  a.SetPose(pose_of(I));
  b.SetPose(pose_of(I));
  c.SetPose(pose_of(I));
  b.mpParent = &a;
  a.mspChildrens.insert(&b);
  b.mspLoopEdges.insert(&c);
  b.mvpOrderedConnectedKeyFrames = {&a, &c};
  b.mvOrderedWeights = {150, 80};
  b.mConnectedKeyFrameWeights[&a] = 150;
  b.mConnectedKeyFrameWeights[&c] = 80;
  REQUIRE(b.GetParent() == &a && a.GetParent() == nullptr && a.hasChild(&b) && !a.hasChild(&c));
  REQUIRE(b.GetLoopEdges().count(&c) == 1 && b.GetWeight(&a) == 150 && b.GetWeight(&b) == 0);
  // (the reference returns an EMPTY list when no weight lies below w: upper_bound reaches end())
  REQUIRE(b.GetCovisiblesByWeight(100).size() == 1 && b.GetCovisiblesByWeight(80).empty());
  REQUIRE(b.GetCovisiblesByWeight(151).empty() && a.GetCovisiblesByWeight(1).empty());
  Map map;
  map.mspKeyFrames = {&a, &b, &c};
  map.mnMaxKFid = 2;
  cv::Mat pos(3, 1, CV_32F);
  for (int k = 0; k < 3; k++) pos.at<float>(k, 0) = 1.f + k;
  MapPoint mp(pos, &b, &map);
  map.mspMapPoints.insert(&mp);
  REQUIRE(map.GetAllKeyFrames().size() == 3 && map.GetAllMapPoints().size() == 1 && map.GetMaxKFid() == 2);
  REQUIRE(mp.GetReferenceKeyFrame() == &b && mp.mnCorrectedByKF == 0 && mp.mnCorrectedReference == 0);
  // the optimiser exists only on a device (no silent fallback)
  LoopClosing::KeyFrameAndPose none;
  std::map<KeyFrame*, std::set<KeyFrame*>> conn;
  bool threw = false;
  try {
    Optimizer::OptimizeEssentialGraph(&map, &a, &c, none, none, conn, true);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  REQUIRE(threw || mp.GetWorldPos().at<float>(0, 0) == 1.f);  // identical poses: the point stays
  std::printf("abi ok\n");
  return 0;
}

static int mode_run(const char* in_path, const char* out_path) {
  Reader in(in_path);
  World W;
  read_world(in, W);
  Optimizer::OptimizeEssentialGraph(&W.map, W.pLoopKF, W.pCurKF, W.NonCorrectedSim3, W.CorrectedSim3, W.LoopConnections,
                                    W.bFixScale);
  FILE* f = std::fopen(out_path, "wb");
  REQUIRE(f);
  for (const auto& kf : W.kfs) {
    const cv::Mat T = kf->GetPose();
    for (int i = 0; i < 12; i++) {
      const float v = T.at<float>(i / 4, i % 4);
      REQUIRE(std::fwrite(&v, 4, 1, f) == 1);
    }
  }
  for (const auto& mp : W.points) {
    const cv::Mat X = mp->GetWorldPos();
    for (int k = 0; k < 3; k++) {
      const float v = X.at<float>(k, 0);
      REQUIRE(std::fwrite(&v, 4, 1, f) == 1);
    }
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "abi") return mode_abi();
  if (argc == 4 && std::string(argv[1]) == "run") return mode_run(argv[2], argv[3]);
  std::fprintf(stderr, "usage: test_essgraph abi | run IN OUT\n");
  return 2;
}

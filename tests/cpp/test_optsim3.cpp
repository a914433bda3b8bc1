// test_optsim3.cpp -- driver of tests/test_optsim3_shim.py: builds KeyFrame / MapPoint object graphs
// from the arrays the Python side wrote and calls the shim's Optimizer::OptimizeSim3 through the
// reference signature (src/Optimizer.cc:1220), writing what the reference's caller sees: the return
// value, g2oS12 and which entries of vpMatches1 are left.
//   test_optsim3 abi             signatures and members; without a device the call throws
//   test_optsim3 run IN OUT      OptimizeSim3 on every graph with the S12 the file gives
//   test_optsim3 chain IN OUT    LoopClosing::ComputeSim3's loop (src/LoopClosing.cc:372-444) without
//                                SearchBySim3: Sim3Solver round-robin, OptimizeSim3 on every returned
//                                Sim3, the first candidate with nInliers >= 20 accepted
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "Objects.h"
#include "Optimizer.h"
#include "Sim3Solver.h"

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
  void sim3(const g2o::Sim3& S) {
    put<double>(S.rotation().x());
    put<double>(S.rotation().y());
    put<double>(S.rotation().z());
    put<double>(S.rotation().w());
    for (int k = 0; k < 3; k++) put<double>(S.translation()[k]);
    put<double>(S.scale());
  }
  void mask(const std::vector<MapPoint*>& v) {
    put<int32_t>((int32_t)v.size());
    for (MapPoint* p : v) put<uint8_t>(p != nullptr);
  }
};

static cv::Mat identity4() {
  cv::Mat T(4, 4, CV_32F);
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) T.at<float>(r, c) = r == c ? 1.f : 0.f;
  return T;
}

static int mode_abi() {
  int (*f)(KeyFrame*, KeyFrame*, std::vector<MapPoint*>&, g2o::Sim3&, const float, const bool) = &Optimizer::OptimizeSim3;
  REQUIRE(f);
  // the g2o::Sim3 slice: R, t, s in; rotation / translation / scale / operator* / inverse / map
  g2o::Matrix3d R;
  R(0, 0) = 0, R(0, 1) = -1, R(0, 2) = 0, R(1, 0) = 1, R(1, 1) = 0, R(1, 2) = 0, R(2, 0) = 0, R(2, 1) = 0, R(2, 2) = 1;
  const g2o::Sim3 S(R, g2o::Vector3d{1., 2., 3.}, 2.0);
  const g2o::Vector3d p = S.map(g2o::Vector3d{1., 0., 0.});
  REQUIRE(std::abs(p[0] - 1.) < 1e-15 && std::abs(p[1] - 4.) < 1e-15 && std::abs(p[2] - 3.) < 1e-15);
  const g2o::Sim3 I = S * S.inverse();
  REQUIRE(std::abs(I.scale() - 1.) < 1e-15 && std::abs(I.rotation().w() - 1.) < 1e-15);
  for (int k = 0; k < 3; k++) REQUIRE(std::abs(I.translation()[k]) < 1e-15);
  const g2o::Matrix3d Rb = S.rotation().toRotationMatrix();
  for (int k = 0; k < 9; k++) REQUIRE(std::abs(Rb.m[k] - R.m[k]) < 1e-15);
  // no matches: nothing is gathered; the optimiser exists only on a device (no silent fallback)
  KeyFrame k1, k2;
  k1.SetPose(identity4());
  k2.SetPose(identity4());
  std::vector<MapPoint*> none(4, nullptr);
  k1.mvpMapPoints = none;
  g2o::Sim3 g = S;
  bool threw = false;
  int n = -1;
  try {
    n = Optimizer::OptimizeSim3(&k1, &k2, none, g, 10.f, false);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  REQUIRE(threw || (n == 0 && g.scale() == 2.0 && g.rotation().w() == S.rotation().w()));  // return 0, g2oS12 kept
  std::printf("abi ok\n");
  return 0;
}

struct Pair {
  std::unique_ptr<KeyFrame> kf1, kf2;
  std::vector<std::unique_ptr<MapPoint>> points;
  std::vector<MapPoint*> vpMatches12;
  bool fix = false;
  float th2 = 0;
  g2o::Sim3 S12;
};

static std::unique_ptr<KeyFrame> read_kf(Reader& in) {
  std::unique_ptr<KeyFrame> kf(new KeyFrame());
  kf->mnId = (long unsigned int)in.get<int64_t>();
  const std::vector<float> T = in.vec<float>(16), K = in.vec<float>(4);
  cv::Mat Tcw(4, 4, CV_32F);
  for (int i = 0; i < 16; i++) Tcw.at<float>(i / 4, i % 4) = T[i];
  kf->SetPose(Tcw);
  kf->fx = K[0], kf->fy = K[1], kf->cx = K[2], kf->cy = K[3];
  const int32_t nk = in.get<int32_t>();
  const std::vector<float> xy = in.vec<float>(2 * (size_t)nk);
  const std::vector<int32_t> oct = in.vec<int32_t>(nk);
  kf->N = nk;
  kf->mvKeysUn.resize(nk);
  for (int i = 0; i < nk; i++) {
    kf->mvKeysUn[i].pt.x = xy[2 * i];
    kf->mvKeysUn[i].pt.y = xy[2 * i + 1];
    kf->mvKeysUn[i].octave = oct[i];
  }
  kf->mvuRight.assign(nk, -1.f);
  kf->mvpMapPoints.assign(nk, nullptr);
  const int32_t nl = in.get<int32_t>();
  kf->mvLevelSigma2 = in.vec<float>(nl);
  kf->mvInvLevelSigma2 = in.vec<float>(nl);
  return kf;
}

static MapPoint* read_point(Reader& in, Pair& P, KeyFrame* kf) {
  if (!in.get<uint8_t>()) return nullptr;
  const std::vector<float> pos = in.vec<float>(3);
  const uint8_t bad = in.get<uint8_t>();
  const int32_t idx = in.get<int32_t>();
  cv::Mat X(3, 1, CV_32F);
  for (int k = 0; k < 3; k++) X.at<float>(k, 0) = pos[k];
  P.points.emplace_back(new MapPoint(X, kf, nullptr));
  MapPoint* mp = P.points.back().get();
  if (idx >= 0) mp->AddObservation(kf, (size_t)idx);
  mp->mbBad = bad != 0;
  return mp;
}

static void read_pair(Reader& in, Pair& P) {
  P.kf1 = read_kf(in);
  P.kf2 = read_kf(in);
  const int32_t n1 = in.get<int32_t>();
  REQUIRE(n1 == P.kf1->N);
  for (int i = 0; i < n1; i++) {
    P.kf1->mvpMapPoints[i] = read_point(in, P, P.kf1.get());
    P.vpMatches12.push_back(read_point(in, P, P.kf2.get()));
  }
  P.fix = in.get<uint8_t>() != 0;
  P.th2 = in.get<float>();
  const std::vector<double> s = in.vec<double>(8);
  P.S12 = g2o::Sim3(g2o::Quaterniond(s[3], s[0], s[1], s[2]), g2o::Vector3d{s[4], s[5], s[6]}, s[7]);
}

static int mode_run(const char* inp, const char* outp) {
  Reader in(inp);
  Writer out(outp);
  const int32_t n = in.get<int32_t>();
  for (int k = 0; k < 3; k++) in.get<int32_t>();  // per_call, max_sweeps, min_inliers: chain mode's
  for (int s = 0; s < n; s++) {
    Pair P;
    read_pair(in, P);
    std::vector<MapPoint*> vpMatches1 = P.vpMatches12;
    g2o::Sim3 g2oS12 = P.S12;
    const int nInliers = Optimizer::OptimizeSim3(P.kf1.get(), P.kf2.get(), vpMatches1, g2oS12, P.th2, P.fix);
    out.put<int32_t>(nInliers);
    out.sim3(g2oS12);
    out.mask(vpMatches1);
  }
  out.put<int32_t>(-1);
  return 0;
}

static int mode_chain(const char* inp, const char* outp) {
  Reader in(inp);
  Writer out(outp);
  const int32_t n = in.get<int32_t>(), per_call = in.get<int32_t>(), max_sweeps = in.get<int32_t>();
  const int32_t min_inliers = in.get<int32_t>();
  std::vector<Pair> pairs(n);
  std::vector<std::unique_ptr<Sim3Solver>> solvers;
  for (int s = 0; s < n; s++) {
    read_pair(in, pairs[s]);
    Pair& P = pairs[s];
    solvers.emplace_back(new Sim3Solver(P.kf1.get(), P.kf2.get(), P.vpMatches12, P.fix));  // src/LoopClosing.cc:355-357
    solvers.back()->SetRansacParameters(0.99, min_inliers, 300);
  }
  std::vector<bool> vbDiscarded(n, false);
  int nCandidates = n;
  bool bMatch = false;
  int matched = -1;
  for (int sweep = 0; sweep < max_sweeps && nCandidates > 0 && !bMatch; sweep++) {
    for (int i = 0; i < n; i++) {
      if (vbDiscarded[i]) continue;
      Pair& P = pairs[i];
      std::vector<bool> vbInliers;
      int nInliers;
      bool bNoMore;
      Sim3Solver* pSolver = solvers[i].get();
      cv::Mat Scm = pSolver->iterate(per_call, bNoMore, vbInliers, nInliers);
      if (bNoMore) {
        vbDiscarded[i] = true;
        nCandidates--;
      }
      out.put<int32_t>(i);
      out.put<uint8_t>(!Scm.empty());
      out.put<uint8_t>(bNoMore);
      if (!Scm.empty()) {  // :404-444 without SearchBySim3
        std::vector<MapPoint*> vpMapPointMatches(P.vpMatches12.size(), static_cast<MapPoint*>(NULL));
        for (size_t j = 0, jend = vbInliers.size(); j < jend; j++)
          if (vbInliers[j]) vpMapPointMatches[j] = P.vpMatches12[j];
        const cv::Mat R = pSolver->GetEstimatedRotation();
        const cv::Mat t = pSolver->GetEstimatedTranslation();
        const float s = pSolver->GetEstimatedScale();
        g2o::Matrix3d Rd;  // Converter::toMatrix3d / toVector3d
        for (int r = 0; r < 3; r++)
          for (int c = 0; c < 3; c++) Rd(r, c) = R.at<float>(r, c);
        g2o::Sim3 gScm(Rd, g2o::Vector3d{t.at<float>(0, 0), t.at<float>(1, 0), t.at<float>(2, 0)}, s);
        const int nOpt = Optimizer::OptimizeSim3(P.kf1.get(), P.kf2.get(), vpMapPointMatches, gScm, 10, P.fix);
        out.put<int32_t>(nOpt);
        out.sim3(gScm);
        out.mask(vpMapPointMatches);
        if (nOpt >= 20) {
          bMatch = true;
          matched = i;
          break;
        }
      }
    }
  }
  out.put<int32_t>(-1);
  out.put<int32_t>(matched);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: test_optsim3 abi | run IN OUT | chain IN OUT\n");
    return 2;
  }
  try {
    const std::string m = argv[1];
    if (m == "abi") return mode_abi();
    if (m == "run" && argc == 4) return mode_run(argv[2], argv[3]);
    if (m == "chain" && argc == 4) return mode_chain(argv[2], argv[3]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "test_optsim3: %s\n", e.what());
    return 1;
  }
  return 2;
}

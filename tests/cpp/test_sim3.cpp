// test_sim3.cpp -- driver of tests/test_sim3_shim.py: builds KeyFrame / MapPoint object graphs from
// the arrays the Python side wrote, constructs the shim's ORB_SLAM2::Sim3Solver through the
// reference signature (include/Sim3Solver.h:40) for every candidate pair, and runs the solver sweep
// of LoopClosing::ComputeSim3 (src/LoopClosing.cc:372-402) with every returned Sim3 treated as one
// that OptimizeSim3 rejects, so the round-robin goes on.  It writes what the reference's caller sees
// after each iterate(): the returned T12, bNoMore, vbInliers, nInliers and the three estimates.
//   test_sim3 abi            signatures and members; without a device the first GPU call throws
//   test_sim3 run IN OUT
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "Objects.h"
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
  void mat(const cv::Mat& m, int rows, int cols) {
    REQUIRE(m.rows == rows && m.cols == cols && m.type() == CV_32F);
    for (int r = 0; r < rows; r++)
      for (int c = 0; c < cols; c++) put<float>(m.at<float>(r, c));
  }
};

static int mode_abi() {
  // the reference's signatures (include/Sim3Solver.h:40-50)
  static_assert(std::is_constructible<Sim3Solver, KeyFrame*, KeyFrame*, const std::vector<MapPoint*>&, bool>::value,
                "ctor");
  static_assert(std::is_constructible<Sim3Solver, KeyFrame*, KeyFrame*, const std::vector<MapPoint*>&>::value,
                "ctor default bFixScale");
  void (Sim3Solver::*p)(double, int, int) = &Sim3Solver::SetRansacParameters;
  cv::Mat (Sim3Solver::*f)(std::vector<bool>&, int&) = &Sim3Solver::find;
  cv::Mat (Sim3Solver::*it)(int, bool&, std::vector<bool>&, int&) = &Sim3Solver::iterate;
  cv::Mat (Sim3Solver::*gr)() = &Sim3Solver::GetEstimatedRotation;
  cv::Mat (Sim3Solver::*gt)() = &Sim3Solver::GetEstimatedTranslation;
  float (Sim3Solver::*gs)() = &Sim3Solver::GetEstimatedScale;
  REQUIRE(p && f && it && gr && gt && gs);
  // an empty match list gathers nothing; the solver exists only on a device (no silent fallback)
  KeyFrame k1, k2;
  cv::Mat T(4, 4, CV_32F);
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) T.at<float>(r, c) = r == c ? 1.f : 0.f;
  k1.SetPose(T);
  k2.SetPose(T);
  std::vector<MapPoint*> none(4, nullptr);
  k1.mvpMapPoints = none;
  Sim3Solver s(&k1, &k2, none, true);
  s.SetRansacParameters(0.99, 20, 300);
  bool threw = false, bNoMore = false;
  std::vector<bool> vb;
  int n = -1;
  try {
    cv::Mat r = s.iterate(5, bNoMore, vb, n);
    REQUIRE(r.empty());
  } catch (const std::runtime_error&) {
    threw = true;
  }
  REQUIRE(threw || (bNoMore && vb.size() == 4 && n == 0));  // N = 0 < 20: bNoMore
  std::printf("abi ok\n");
  return 0;
}

struct Pair {
  std::unique_ptr<KeyFrame> kf1, kf2;
  std::vector<std::unique_ptr<MapPoint>> points;
  std::vector<MapPoint*> vpMatched12;
  bool fix = false;
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
  const std::vector<int32_t> oct = in.vec<int32_t>(nk);
  kf->N = nk;
  kf->mvKeysUn.resize(nk);
  for (int i = 0; i < nk; i++) kf->mvKeysUn[i].octave = oct[i];
  kf->mvuRight.assign(nk, -1.f);
  kf->mvpMapPoints.assign(nk, nullptr);
  const int32_t nl = in.get<int32_t>();
  kf->mvLevelSigma2 = in.vec<float>(nl);
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

static int mode_run(const char* inp, const char* outp) {
  Reader in(inp);
  Writer out(outp);
  const int32_t n = in.get<int32_t>(), per_call = in.get<int32_t>(), max_sweeps = in.get<int32_t>();
  const int32_t min_inliers = in.get<int32_t>();
  std::vector<Pair> pairs(n);
  std::vector<std::unique_ptr<Sim3Solver>> solvers;
  for (int s = 0; s < n; s++) {
    Pair& P = pairs[s];
    P.kf1 = read_kf(in);
    P.kf2 = read_kf(in);
    const int32_t n1 = in.get<int32_t>();
    REQUIRE(n1 == P.kf1->N);
    for (int i = 0; i < n1; i++) {
      P.kf1->mvpMapPoints[i] = read_point(in, P, P.kf1.get());   // vpKeyFrameMP1[i1]
      P.vpMatched12.push_back(read_point(in, P, P.kf2.get()));   // vpMatched12[i1]
    }
    P.fix = in.get<uint8_t>() != 0;
    // src/LoopClosing.cc:355-357
    solvers.emplace_back(new Sim3Solver(P.kf1.get(), P.kf2.get(), P.vpMatched12, P.fix));
    solvers.back()->SetRansacParameters(0.99, min_inliers, 300);
  }
  // src/LoopClosing.cc:372-402, every returned Sim3 rejected by the (absent) OptimizeSim3
  std::vector<bool> vbDiscarded(n, false);
  int nCandidates = n;
  for (int sweep = 0; sweep < max_sweeps && nCandidates > 0; sweep++) {
    for (int i = 0; i < n; i++) {
      if (vbDiscarded[i]) continue;
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
      out.put<int32_t>(nInliers);
      out.put<int32_t>((int32_t)vbInliers.size());
      for (bool b : vbInliers) out.put<uint8_t>(b);
      if (!Scm.empty()) out.mat(Scm, 4, 4);
      out.mat(pSolver->GetEstimatedRotation(), 3, 3);
      out.mat(pSolver->GetEstimatedTranslation(), 3, 1);
      out.put<float>(pSolver->GetEstimatedScale());
    }
  }
  out.put<int32_t>(-1);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: test_sim3 abi | run IN OUT\n");
    return 2;
  }
  try {
    const std::string m = argv[1];
    if (m == "abi") return mode_abi();
    if (m == "run" && argc == 4) return mode_run(argv[2], argv[3]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "test_sim3: %s\n", e.what());
    return 1;
  }
  return 2;
}

// test_covis.cpp -- driver of tests/test_covis_shim.py: replays a list of operations on the shim's KeyFrame /
// MapPoint / Map / LocalMapping objects through the reference's signatures -- KeyFrame::UpdateConnections()
// (include/KeyFrame.h:71) and LocalMapping::KeyFrameCulling() (include/LocalMapping.h:106) -- and writes what the
// reference's callers would see: mConnectedKeyFrameWeights, the ordered vectors, parent, children and isBad()
// of every keyframe, isBad() of every point.
//   test_covis abi            no GPU: signatures, members, host-side graph calls, loud failure without a device
//   test_covis run IN OUT     IN: operations (u32 opcode ...), 0 ends; OUT: int64 words
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "LocalMapping.h"
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
  void put(int64_t v) { REQUIRE(std::fwrite(&v, sizeof(v), 1, f) == 1); }
};

static int mode_abi() {
  // the reference's signatures (include/KeyFrame.h:66-134, include/LocalMapping.h:106)
  void (KeyFrame::*uc)() = &KeyFrame::UpdateConnections;
  void (KeyFrame::*ac)(KeyFrame*, const int&) = &KeyFrame::AddConnection;
  void (KeyFrame::*ec)(KeyFrame*) = &KeyFrame::EraseConnection;
  void (KeyFrame::*ub)() = &KeyFrame::UpdateBestCovisibles;
  void (KeyFrame::*ach)(KeyFrame*) = &KeyFrame::AddChild;
  void (KeyFrame::*cp)(KeyFrame*) = &KeyFrame::ChangeParent;
  void (KeyFrame::*sb)() = &KeyFrame::SetBadFlag;
  void (LocalMapping::*kc)() = &LocalMapping::KeyFrameCulling;
  REQUIRE(uc && ac && ec && ub && ach && cp && sb && kc);
  // the host-side graph calls: weights 5, 5, 7 -> ordered 7, then the two 5s in descending id
  KeyFrame a, b, c, d;
  a.mnId = 1, b.mnId = 2, c.mnId = 3, d.mnId = 4;
  a.AddConnection(&b, 5);
  a.AddConnection(&c, 5);
  a.AddConnection(&d, 7);
  REQUIRE((a.GetVectorCovisibleKeyFrames() == std::vector<KeyFrame*>{&d, &c, &b}));
  REQUIRE((a.mvOrderedWeights == std::vector<int>{7, 5, 5}) && a.GetWeight(&c) == 5);
  a.EraseConnection(&d);
  REQUIRE((a.GetVectorCovisibleKeyFrames() == std::vector<KeyFrame*>{&c, &b}));
  b.ChangeParent(&a);
  REQUIRE(b.GetParent() == &a && a.hasChild(&b) && a.GetChilds().size() == 1);
  // no Map, and no device behind a Map: UpdateConnections and KeyFrameCulling throw (no silent fallback)
  bool threw = false;
  try {
    a.UpdateConnections();
  } catch (const std::runtime_error&) {
    threw = true;
  }
  REQUIRE(threw);
  Map map;
  a.mpMap = &map;
  int fails = 0;
  try {
    a.UpdateConnections();
  } catch (const std::runtime_error&) {
    fails++;
  }
  LocalMapping lm(&map, 1.f);
  lm.mpCurrentKeyFrame = &a;
  try {
    lm.KeyFrameCulling();
  } catch (const std::runtime_error&) {
    fails++;
  }
  // with a device both fail too: the table does not hold keyframe 1 (nothing was uploaded)
  REQUIRE(fails == 2);
  std::printf("abi ok\n");
  return 0;
}

static int mode_run(const char* in, const char* out) {
  Reader R(in);
  Writer W(out);
  Map map;
  std::map<int64_t, std::unique_ptr<KeyFrame>> kfs;
  std::map<int64_t, std::unique_ptr<MapPoint>> mps;
  auto kf = [&](int64_t id) {
    std::unique_ptr<KeyFrame>& p = kfs[id];
    if (!p) {
      p.reset(new KeyFrame());
      p->mnId = (long unsigned int)id;
      p->mpMap = &map;
      p->mThDepth = 2.0f;
      map.AddKeyFrame(p.get());
    }
    return p.get();
  };
  auto mp = [&](int64_t id) {
    std::unique_ptr<MapPoint>& p = mps[id];
    if (!p) {
      p.reset(new MapPoint());
      p->mnId = (long unsigned int)id;
      p->mpMap = &map;
      map.AddMapPoint(p.get());
    }
    return p.get();
  };
  auto dump = [&]() {
    W.put((int64_t)kfs.size());
    for (auto& e : kfs) {
      KeyFrame* k = e.second.get();
      W.put(e.first);
      W.put(k->isBad() ? 1 : 0);
      W.put(k->GetParent() ? (int64_t)k->GetParent()->mnId : -1);
      std::map<int64_t, int> w;
      for (auto& m : k->mConnectedKeyFrameWeights) w[(int64_t)m.first->mnId] = m.second;
      W.put((int64_t)w.size());
      for (auto& m : w) {
        W.put(m.first);
        W.put(m.second);
      }
      const std::vector<KeyFrame*> ord = k->GetVectorCovisibleKeyFrames();
      W.put((int64_t)ord.size());
      for (KeyFrame* o : ord) W.put((int64_t)o->mnId);
      W.put((int64_t)k->mvOrderedWeights.size());
      for (int x : k->mvOrderedWeights) W.put(x);
      std::vector<int64_t> ch;
      for (KeyFrame* c : k->GetChilds()) ch.push_back((int64_t)c->mnId);
      std::sort(ch.begin(), ch.end());
      W.put((int64_t)ch.size());
      for (int64_t c : ch) W.put(c);
    }
    W.put((int64_t)mps.size());
    for (auto& e : mps) {
      W.put(e.first);
      W.put(e.second->isBad() ? 1 : 0);
    }
  };
  for (;;) {
    const uint32_t op = R.get<uint32_t>();
    if (op == 0) break;
    if (op == 1) {  // a keyframe's row, as ProcessNewKeyFrame leaves the objects; then the upload helper
      KeyFrame* k = kf(R.get<int64_t>());
      const int32_t n = R.get<int32_t>();
      const std::vector<int32_t> pid = R.vec<int32_t>(n), oct = R.vec<int32_t>(n);
      const std::vector<float> uR = R.vec<float>(n), depth = R.vec<float>(n);
      for (size_t i = 0; i < k->mvpMapPoints.size(); i++)  // the old row's observations leave (no nObs <= 2 test)
        if (MapPoint* p = k->mvpMapPoints[i])
          if (!p->isBad() && p->mObservations.count(k)) {
            p->nObs -= k->mvuRight[i] >= 0 ? 2 : 1;
            p->mObservations.erase(k);
          }
      k->N = n;
      k->mvKeysUn.assign(n, cv::KeyPoint());
      for (int i = 0; i < n; i++) k->mvKeysUn[i].octave = oct[i];
      k->mvuRight = uR;
      k->mvDepth = depth;
      k->mvpMapPoints.assign(n, nullptr);
      for (int i = 0; i < n; i++) {
        if (pid[i] < 0) continue;
        MapPoint* p = mp(pid[i]);
        if (p->isBad()) continue;
        k->AddMapPoint(p, i);
        p->AddObservation(k, i);
      }
      map.UploadCovisibilityRow(k);
    } else if (op == 2) {  // MapPoint::SetBadFlag, reported to the table
      const int32_t n = R.get<int32_t>();
      std::vector<MapPoint*> v;
      for (int32_t id : R.vec<int32_t>(n)) {
        mp(id)->SetBadFlag();
        v.push_back(mp(id));
      }
      map.CovisibilityPointsBad(v);
    } else if (op == 3) {  // KeyFrame::UpdateConnections()
      kf(R.get<int64_t>())->UpdateConnections();
      dump();
    } else if (op == 4) {  // LocalMapping::KeyFrameCulling() for a current keyframe with these covisibles
      const int32_t n = R.get<int32_t>();
      const std::vector<int64_t> ids = R.vec<int64_t>(n);
      const std::vector<uint8_t> ne = R.vec<uint8_t>(n);
      const int32_t mono = R.get<int32_t>();
      KeyFrame cur;
      cur.mnId = 1000000;
      for (int i = 0; i < n; i++) {
        KeyFrame* k = kf(ids[i]);
        k->mbNotErase = ne[i] != 0;
        cur.mvpOrderedConnectedKeyFrames.push_back(k);
      }
      LocalMapping lm(&map, mono ? 1.f : 0.f);
      lm.mpCurrentKeyFrame = &cur;
      lm.KeyFrameCulling();
      dump();
    } else {
      REQUIRE(!"unknown opcode");
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: test_covis abi | run IN OUT\n");
    return 2;
  }
  const std::string m = argv[1];
  try {
    if (m == "abi") return mode_abi();
    if (m == "run" && argc >= 4) return mode_run(argv[2], argv[3]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 3;
  }
  return 2;
}

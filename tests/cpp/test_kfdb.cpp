// test_kfdb.cpp -- driver of tests/test_kfdb_shim.py: replays a list of operations on the shim's
// ORB_SLAM2::KeyFrameDatabase through the reference signatures (include/KeyFrameDatabase.h) on
// KeyFrame / Frame objects it builds from the arrays the Python side wrote, and writes what the
// reference's callers would see: the candidates' mnIds, ORBVocabulary::score doubles, and the six
// KeyFrame members the queries write.
//   test_kfdb abi            no GPU: signatures, members, loud failure without a device
//   test_kfdb run IN OUT     IN: u64 len + vocabulary text, then operations (u32 opcode ...), 0 ends
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "KeyFrameDatabase.h"
#include "ORBVocabulary.h"
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
  DBoW2::BowVector bow() {
    const int32_t n = get<int32_t>();
    const std::vector<uint32_t> w = vec<uint32_t>(n);
    const std::vector<double> x = vec<double>(n);
    DBoW2::BowVector b;
    for (int i = 0; i < n; i++) b[w[i]] = x[i];
    return b;
  }
};

struct Writer {
  FILE* f;
  explicit Writer(const char* p) : f(std::fopen(p, "wb")) { REQUIRE(f); }
  ~Writer() { std::fclose(f); }
  template <class T> void put(T v) { REQUIRE(std::fwrite(&v, sizeof(T), 1, f) == 1); }
  void ids(const std::vector<KeyFrame*>& v) {
    put<int32_t>((int32_t)v.size());
    for (KeyFrame* k : v) put<int64_t>((int64_t)k->mnId);
  }
};

static int mode_abi() {
  // the reference's signatures (include/KeyFrameDatabase.h:46-62, include/KeyFrame.h:75,79,181-194)
  static_assert(std::is_constructible<KeyFrameDatabase, const ORBVocabulary&>::value, "ctor");
  void (KeyFrameDatabase::*a)(KeyFrame*) = &KeyFrameDatabase::add;
  void (KeyFrameDatabase::*e)(KeyFrame*) = &KeyFrameDatabase::erase;
  void (KeyFrameDatabase::*c)() = &KeyFrameDatabase::clear;
  std::vector<KeyFrame*> (KeyFrameDatabase::*l)(KeyFrame*, float) = &KeyFrameDatabase::DetectLoopCandidates;
  std::vector<KeyFrame*> (KeyFrameDatabase::*r)(Frame*) = &KeyFrameDatabase::DetectRelocalizationCandidates;
  double (ORBVocabulary::*s)(const DBoW2::BowVector&, const DBoW2::BowVector&) const = &ORBVocabulary::score;
  REQUIRE(a && e && c && l && r && s);
  KeyFrame k, k2, k3;
  static_assert(std::is_same<decltype(k.mnLoopQuery), long unsigned int>::value, "mnLoopQuery");
  static_assert(std::is_same<decltype(k.mnRelocQuery), long unsigned int>::value, "mnRelocQuery");
  static_assert(std::is_same<decltype(k.mnLoopWords), int>::value && std::is_same<decltype(k.mLoopScore), float>::value,
                "loop members");
  static_assert(std::is_same<decltype(k.mnRelocWords), int>::value &&
                    std::is_same<decltype(k.mRelocScore), float>::value,
                "reloc members");
  REQUIRE(k.mnLoopQuery == 0 && k.mnLoopWords == 0 && k.mnRelocQuery == 0 && k.mnRelocWords == 0);
  k.mvpOrderedConnectedKeyFrames = {&k2, &k3};
  REQUIRE(k.GetBestCovisibilityKeyFrames(10).size() == 2 && k.GetBestCovisibilityKeyFrames(1)[0] == &k2);
  REQUIRE(k.GetConnectedKeyFrames().count(&k3) == 1);
  // no vocabulary on a device: the constructor and score throw (no silent fallback)
  ORBVocabulary voc;
  bool threw = false;
  try {
    KeyFrameDatabase db(voc);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  REQUIRE(threw);
  threw = false;
  try {
    (void)voc.score(DBoW2::BowVector(), DBoW2::BowVector());
  } catch (const std::runtime_error&) {
    threw = true;
  }
  REQUIRE(threw);
  std::printf("abi ok\n");
  return 0;
}

static int mode_run(const char* in, const char* out) {
  Reader R(in);
  Writer W(out);
  const uint64_t len = R.get<uint64_t>();
  const std::vector<char> text = R.vec<char>(len);
  ORBVocabulary voc;
  REQUIRE(voc.loadFromText(std::string(text.begin(), text.end())));
  KeyFrameDatabase db(voc);
  std::map<int64_t, std::unique_ptr<KeyFrame>> kfs;
  auto kf = [&](int64_t id) {
    std::unique_ptr<KeyFrame>& p = kfs[id];
    if (!p) {
      p.reset(new KeyFrame());
      p->mnId = (long unsigned int)id;
    }
    return p.get();
  };
  for (;;) {
    const uint32_t op = R.get<uint32_t>();
    if (op == 0) break;
    if (op == 1) {  // add
      KeyFrame* k = kf(R.get<int64_t>());
      k->mBowVec = R.bow();
      db.add(k);
    } else if (op == 2) {  // erase
      db.erase(kf(R.get<int64_t>()));
    } else if (op == 3) {  // covisibility lists
      const int32_t n = R.get<int32_t>();
      for (int i = 0; i < n; i++) {
        KeyFrame* k = kf(R.get<int64_t>());
        const int32_t nb = R.get<int32_t>();
        k->mvpOrderedConnectedKeyFrames.clear();
        for (int64_t id : R.vec<int64_t>(nb)) k->mvpOrderedConnectedKeyFrames.push_back(kf(id));
      }
    } else if (op == 4) {  // DetectRelocalizationCandidates(Frame*)
      Frame F;
      F.mnId = (long unsigned int)R.get<uint64_t>();
      F.mBowVec = R.bow();
      W.ids(db.DetectRelocalizationCandidates(&F));
    } else if (op == 5) {  // DetectLoopCandidates(KeyFrame*, float)
      KeyFrame* k = kf((int64_t)R.get<uint64_t>());
      k->mBowVec = R.bow();
      const int32_t nc = R.get<int32_t>();
      k->mvpOrderedConnectedKeyFrames.clear();
      for (int64_t id : R.vec<int64_t>(nc)) k->mvpOrderedConnectedKeyFrames.push_back(kf(id));
      const float min_score = R.get<float>();
      W.ids(db.DetectLoopCandidates(k, min_score));
    } else if (op == 6) {  // ORBVocabulary::score(query, pKF->mBowVec)
      const DBoW2::BowVector q = R.bow();
      const int32_t n = R.get<int32_t>();
      for (int64_t id : R.vec<int64_t>(n)) W.put<double>(voc.score(q, kf(id)->mBowVec));
    } else if (op == 7) {  // the members as the reference's code reads them
      const int32_t n = R.get<int32_t>();
      for (int64_t id : R.vec<int64_t>(n)) {
        KeyFrame* k = kf(id);
        W.put<uint64_t>(k->mnRelocQuery);
        W.put<int32_t>(k->mnRelocWords);
        W.put<float>(k->mRelocScore);
        W.put<uint64_t>(k->mnLoopQuery);
        W.put<int32_t>(k->mnLoopWords);
        W.put<float>(k->mLoopScore);
      }
    } else {
      REQUIRE(!"unknown opcode");
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: test_kfdb abi | run IN OUT\n");
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

// test_staging.cpp -- the layout phase of orbx::Staging (csrc/orbx_scratch.h), on the host alone:
// no HIP call is made, so it runs without a device (tests/test_staging.py builds it with the
// address and undefined-behaviour sanitizers and runs it as a child process).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../orb_slam2_commit_amd/csrc/orbx_scratch.h"

using orbx::Staging;
using Out = Staging::Outputs;

static int g_checks = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    g_checks++;                                                   \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

struct Span {
  size_t off, bytes;
};
template <class T>
static Span span(Staging::Slot<T> s) {
  return {s.off, s.count * sizeof(T)};
}
// declaration order is offset order, 256-aligned, no two slots share a byte
static void check_ordered(const std::vector<Span>& v) {
  size_t end = 0;
  for (const Span& s : v) {
    CHECK(s.off % 256 == 0);
    CHECK(s.off >= end);
    end = s.off + s.bytes;
  }
}

struct Rec {
  void* p[9];
  int n;
};

static void test_ordering_and_odd_sizes() {
  const uint8_t flags[37] = {};
  const orbx_keypoint kps[3] = {};
  const float f[5] = {};
  Staging S(0);
  const auto a = S.in(flags, 37);  // 37 B
  const auto b = S.in(kps, 3);     // 84 B
  const auto c = S.in(f, 5);       // 20 B
  const auto r = S.record<Rec>();
  const auto o1 = S.out<int32_t>(37);
  const auto o2 = S.out<uint8_t>(1);
  const auto o3 = S.inout(f, 5);
  const auto d1 = S.device_only<double>(33);
  const auto d2 = S.device_only<int>(3);
  check_ordered({span(a), span(b), span(c), span(r), span(o1), span(o2), span(o3), span(d1), span(d2)});
  CHECK(a.off == 0 && b.off == 256 && c.off == 512 && r.off == 768);
  CHECK(sizeof(orbx_keypoint) == 28 && b.count * sizeof(orbx_keypoint) == 84);
  // the ranges: upload by mode, download exactly the outputs
  CHECK(S.outputs_begin() == o1.off);
  CHECK(S.outputs_end() == d1.off);
  CHECK(S.upload_bytes(Out::skipped) == o1.off);
  CHECK(S.upload_bytes(Out::zeroed) == d1.off);
  CHECK(r.off + sizeof(Rec) <= S.outputs_begin());  // the descriptor goes up in either mode
  CHECK(o3.off + 20 <= S.outputs_end());
  // the device-only bytes lie in neither range and have no pinned bytes; the device size covers them
  CHECK(d1.off >= S.upload_bytes(Out::zeroed) && d1.off >= S.outputs_end());
  CHECK(S.pinned_bytes() == d1.off);
  CHECK(S.device_bytes() >= d2.off + 3 * sizeof(int));
  CHECK(S.device_bytes() > S.pinned_bytes());
  CHECK(S.device_bytes() % 256 == 0);
}

static void test_zero_counts() {
  const float f[70] = {};
  size_t with[4], without[4];
  for (int pass = 0; pass < 2; pass++) {
    Staging S(0);
    size_t* o = pass ? with : without;
    o[0] = S.in(f, 70).off;
    if (pass) {
      const auto z = S.in(f, 0);
      CHECK(z.count == 0 && z.off % 256 == 0);
      CHECK(S.in((const uint8_t*)nullptr, 0).count == 0);
    }
    o[1] = S.in(f, 3).off;
    if (pass) S.record<Rec>(0);
    o[2] = S.out<float>(70).off;
    if (pass) S.out<double>(0);
    o[3] = S.out<float>(1).off;
    if (pass) S.device_only<double>(0);
    CHECK(S.device_bytes() == o[3] + 256 && S.pinned_bytes() == S.device_bytes());
    CHECK(S.outputs_begin() == o[2]);
  }
  for (int k = 0; k < 4; k++) CHECK(with[k] == without[k]);
  Staging E(0);  // nothing at all is legal too
  CHECK(E.device_bytes() == 0 && E.pinned_bytes() == 0 && E.upload_bytes(Out::zeroed) == 0);
}

static void test_optional_inputs() {
  const float f[9] = {};
  Staging S(0);
  const auto a = S.in(f, 9);
  const auto none = S.in_opt((const float*)nullptr, 1000);
  const auto some = S.in_opt(f, 9);
  const auto b = S.in(f, 9);
  CHECK(!none.present && none.count == 0);
  CHECK(S.dev(none) == nullptr);
  CHECK(a.off == 0 && some.off == 256 && b.off == 512);  // the absent one took no bytes
  CHECK(some.present && some.count == 9);
  CHECK(S.dev(Staging::Slot<int>{}) == nullptr);  // a slot never declared (a kind without the array)
}

// two problems one after the other, region by region (SearchBySim3's two directions)
static void test_two_problems() {
  const uint8_t d[3 * 32] = {};
  const float x[15] = {};
  Staging S(0);
  std::vector<Span> all;
  const int nf[2] = {3, 1}, np[2] = {5, 2};
  for (int z = 0; z < 2; z++) {
    all.push_back(span(S.in(d, (size_t)nf[z] * 32)));
    all.push_back(span(S.in_opt(z ? nullptr : x, (size_t)np[z] * 3)));
    all.push_back(span(S.in(x, (size_t)np[z] * 2)));
  }
  const size_t in_end = S.device_bytes();
  const auto rec = S.record<Rec>(2);
  all.push_back(span(rec));
  const size_t out_begin = S.device_bytes();
  for (int z = 0; z < 2; z++) {
    all.push_back(span(S.out<int32_t>((size_t)nf[z])));
    all.push_back(span(S.out<int32_t>((size_t)np[z])));
    all.push_back(span(S.out<int32_t>(1)));
  }
  const size_t out_end = S.device_bytes();
  const auto split = S.device_only<uint8_t>(2 * 1000);
  all.push_back(span(split));
  check_ordered(all);
  CHECK(rec.off == in_end);  // inputs are one range from 0, the records right behind them
  CHECK(S.outputs_begin() == out_begin && S.outputs_end() == out_end);
  CHECK(S.upload_bytes(Out::zeroed) == out_end && S.upload_bytes(Out::skipped) == out_begin);
  CHECK(split.off == out_end && S.pinned_bytes() == out_end);
  CHECK(S.device_bytes() == out_end + orbx::scratch_align(2000));
}

static void test_order_violations() {
  const float f[4] = {};
  {
    Staging S(0);  // an input after an output
    S.in(f, 4);
    S.out<float>(4);
    S.in(f, 4);
    CHECK(S.commit() == ORBX_ERR_ARG);
  }
  {
    Staging S(0);  // an optional input without a source still has a place in the order
    S.out<float>(4);
    S.in_opt((const float*)nullptr, 4);
    CHECK(S.commit() == ORBX_ERR_ARG);
  }
  {
    Staging S(0);  // a descriptor after an output
    S.in(f, 4);
    S.out<float>(4);
    S.record<Rec>();
    CHECK(S.commit() == ORBX_ERR_ARG);
  }
  {
    Staging S(0);  // an input after a descriptor
    S.record<Rec>();
    S.in(f, 4);
    CHECK(S.commit() == ORBX_ERR_ARG);
  }
  for (int what = 0; what < 4; what++) {  // anything after a device-only slot
    Staging S(0);
    S.in(f, 4);
    S.device_only<double>(8);
    if (what == 0) S.in(f, 4);
    if (what == 1) S.record<Rec>();
    if (what == 2) S.out<float>(4);
    if (what == 3) S.inout(f, 4);
    CHECK(S.commit() == ORBX_ERR_ARG);
    CHECK(S.commit() == ORBX_ERR_ARG);  // sticky
  }
}

int main() {
  CHECK(orbx::scratch_align(0) == 0 && orbx::scratch_align(1) == 256 && orbx::scratch_align(256) == 256 &&
        orbx::scratch_align(257) == 512);
  test_ordering_and_odd_sizes();
  test_zero_counts();
  test_optional_inputs();
  test_two_problems();
  test_order_violations();
  std::printf("staging layout ok: %d checks\n", g_checks);
  return 0;
}

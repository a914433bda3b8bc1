// test_mem.cpp -- the owners of csrc/orbx_mem.h where the GPU suite never goes: every allocation
// fails.  Run without a visible device (tests/test_mem.py builds it with the address and
// undefined-behaviour sanitizers and runs it as a child process only when there is no GPU): a failed
// ensure leaves the owner empty, and everything done to an empty owner afterwards is safe -- the
// address sanitizer is the judge of double frees.  Then the sites' growth policies, held to the
// expressions they replaced, written out as numbers.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../orb_slam2_commit_amd/csrc/orbx_scratch.h"  // (brings orbx_mem.h; lease_capacity, arena_capacity)

using orbx::DevBuf;
using orbx::PinnedBuf;

static int g_checks = 0;
#define CHECK(c)                                               \
  do {                                                         \
    g_checks++;                                                \
    if (!(c)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                            \
    }                                                          \
  } while (0)

static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value, "");
static_assert(!std::is_copy_constructible<PinnedBuf>::value && !std::is_copy_assignable<PinnedBuf>::value, "");
static_assert(std::is_nothrow_move_constructible<DevBuf<int>>::value, "");
static_assert(std::is_nothrow_move_constructible<PinnedBuf>::value, "");
static_assert(!std::is_copy_constructible<orbx::Event>::value && !std::is_copy_constructible<orbx::Stream>::value, "");

template <class T>
static bool empty(const DevBuf<T>& b) {
  return b.p == nullptr && b.n == 0;
}
static bool empty(const PinnedBuf& b) { return b.p == nullptr && b.cap == 0 && b.dev() == nullptr; }

static void dev_buf_failures() {
  DevBuf<double> a;
  CHECK(empty(a));
  CHECK(a.ensure(100) != hipSuccess);
  CHECK(empty(a));
  CHECK(a.ensure(0) != hipSuccess);  // (an empty owner allocates even for a count of zero)
  CHECK(empty(a));
  const std::vector<double> v(7, 1.0);
  CHECK(a.upload(v) != hipSuccess);
  CHECK(a.upload(v.data(), v.size()) != hipSuccess);
  CHECK(empty(a));
  a.release();
  a.release();
  CHECK(empty(a));
  DevBuf<double> b(std::move(a));  // move-from, both ways
  CHECK(empty(a) && empty(b));
  a = std::move(b);
  CHECK(empty(a) && empty(b));
  DevBuf<double> c;
  a.swap(c);
  CHECK(empty(a) && empty(c));
  CHECK(c.ensure(1) != hipSuccess);
  CHECK(empty(c));
}  // three destructors

static void pinned_buf_failures(bool mapped) {
  PinnedBuf a(mapped);
  CHECK(a.mapped() == mapped && empty(a));
  CHECK(a.ensure(1000) != hipSuccess);
  CHECK(empty(a));  // (the mapped mode reports no device pointer)
  CHECK(a.as<int>() == nullptr && a.dev<int>() == nullptr);
  CHECK(a.ensure(0) != hipSuccess);
  CHECK(empty(a));
  a.release();
  a.release();
  PinnedBuf b(std::move(a));
  CHECK(b.mapped() == mapped && empty(a) && empty(b));
  PinnedBuf c(!mapped);
  c = std::move(b);
  CHECK(c.mapped() == mapped && empty(b) && empty(c));
  PinnedBuf d(mapped);
  c.swap(d);
  CHECK(empty(c) && empty(d));
  CHECK(d.ensure(sizeof(int)) != hipSuccess);
  CHECK(empty(d));
}

static void event_stream_failures() {
  orbx::Event e;
  CHECK(e.ensure() != hipSuccess);
  CHECK(e.ev == nullptr && (hipEvent_t)e == nullptr);
  CHECK(e.ensure(hipEventDefault) != hipSuccess);
  CHECK(e.ev == nullptr);
  orbx::Stream s;
  CHECK(s.ensure() != hipSuccess);
  CHECK(s.st == nullptr && (hipStream_t)s == nullptr);
}

// a lease's reserve is the first user of the owners on the call path
static void lease_failure() {
  orbx::ScratchLease l;
  CHECK(l.reserve(1000, 1000) != hipSuccess);
  CHECK(l.d == nullptr && l.h == nullptr && empty(l.dmem) && empty(l.hmem));
  CHECK(l.reserve(0, 0) != hipSuccess);
  CHECK(l.d == nullptr && l.h == nullptr);
}

static void growth_policies() {
  const size_t size[9] = {0, 1, 255, 256, 257, 4095, 4096, 4097, (size_t)1 << 20};
  // the extractor's whole pages, (bytes + 4095) & ~4095 -- but never nothing: that expression's 0 for 0 is one page
  const size_t pages[9] = {4096, 4096, 4096, 4096, 4096, 4096, 4096, 8192, 1048576};
  // the lease: scratch_align(bytes + bytes / 4)
  const size_t lease[9] = {0, 256, 512, 512, 512, 5120, 5120, 5376, 1310720};
  // the LocalBA arenas: bytes + bytes / 4 + 4096
  const size_t arena[9] = {4096, 4097, 4414, 4416, 4417, 9214, 9216, 9217, 1314816};
  for (int i = 0; i < 9; i++) {
    CHECK(orbx::pinned_pages(size[i]) == pages[i]);
    CHECK(orbx::lease_capacity(size[i]) == lease[i]);
    CHECK(orbx::arena_capacity(size[i]) == arena[i]);
    // what the pinned owner makes of a site's padded figure is never less than the figure
    CHECK(orbx::pinned_pages(lease[i]) >= lease[i] && orbx::pinned_pages(arena[i]) >= arena[i]);
  }
  // A pinned block and its device twin (the LocalBA arenas): the pinned owner holds whole pages, the twin
  // exactly what was asked, and the pair counts as holding the smaller of the two -- so a request between
  // the two capacities grows the pair.  reserve(1000) leaves 5346 device bytes under 8192 pinned ones;
  // reserve(6000) must not be a no-op.
  CHECK(orbx::pinned_pages(orbx::arena_capacity(1000)) == 8192 && orbx::arena_capacity(1000) == 5346);
  CHECK(orbx::pair_capacity(8192, 5346, false) == 5346);
  CHECK(!(6000 <= orbx::pair_capacity(8192, 5346, false)));
  CHECK(orbx::pair_capacity(8192, 0, true) == 8192);    // mapped: no twin, the pinned block alone
  CHECK(orbx::pair_capacity(0, 0, false) == 0 && orbx::pair_capacity(0, 0, true) == 0);  // after a failure
  CHECK(orbx::pair_capacity(4096, 8192, false) == 4096);
  for (int i = 0; i < 9; i++) {
    const size_t pinned = orbx::pinned_pages(arena[i]), twin = arena[i];  // what reserve(size[i]) leaves
    CHECK(orbx::pair_capacity(pinned, twin, false) == twin && twin >= size[i]);
    CHECK(orbx::pair_capacity(pinned, 0, true) == pinned && pinned >= size[i]);
    // every request the pair accepts without growing fits both sides
    CHECK(orbx::pair_capacity(pinned, twin, false) <= pinned && orbx::pair_capacity(pinned, twin, false) <= twin);
  }
  static_assert(orbx::scratch_align(257) == 512 && orbx::lease_capacity(1) == 256, "usable in constant expressions");
}

int main() {
  growth_policies();
  dev_buf_failures();
  pinned_buf_failures(false);
  pinned_buf_failures(true);
  event_stream_failures();
  lease_failure();
  std::printf("mem owners ok (%d checks)\n", g_checks);
  return 0;
}

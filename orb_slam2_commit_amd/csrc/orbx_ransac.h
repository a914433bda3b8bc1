// orbx_ransac.h -- host scaffolding shared by the RANSAC solvers (pnp.hip, sim3.hip): the
// per-device context, minimal-set sampling on the caller's rand() values, and the peek /
// advance pair on an orbx_rand_state.  Host only; each solver family keeps its own contexts.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "../../include/orbx.h"
#include "orbx_scratch.h"

namespace orbx {


#define RANSAC_CHECK(x)                          \
  do {                                           \
    if ((x) != hipSuccess) return ORBX_ERR_HIP;  \
  } while (0)

// One stream, one pinned block and one device staging block per device and solver family, shared
// by every solver of the family (the reference creates a solver per candidate, so creation must
// be cheap).  Both blocks only grow.  The contexts live for the process: a family keeps its array
// behind a pointer it never deletes (orbx_mem.h), so nothing here is freed at exit.
struct RansacDevice {
  std::once_flag once;
  hipError_t init_err = hipSuccess;
  hipStream_t st = nullptr;
  std::mutex mu;  // serialises the calls that share the stream and the two blocks
  void* pinned = nullptr;  // pinned_mem's block
  void* dstage = nullptr;  // dstage_mem's block, the device side of the batched calls: job records, sets, results
  PinnedBuf pinned_mem;
  DevBuf<uint8_t> dstage_mem;
  hipError_t dstage_reserve(size_t bytes) {
    if (bytes <= dstage_mem.n) return hipSuccess;  // (also zero bytes of a fresh context: nothing is allocated)
    const hipError_t e = dstage_mem.ensure(bytes);
    dstage = dstage_mem.p;
    return e;
  }
  hipError_t pinned_reserve(size_t bytes) {
    if (bytes <= pinned_mem.cap) return hipSuccess;
    const hipError_t e = pinned_mem.ensure(bytes);
    pinned = pinned_mem.p;
    return e;
  }
};

// Selects `device` and initialises devs[device] on first use; kernel_setup (may be null) runs
// once after the stream exists, for the family's hipFuncSetAttribute calls.
inline orbx_status ransac_device_check(RansacDevice* devs, int device, hipError_t (*kernel_setup)()) {
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return ORBX_ERR_NODEV;
  if (device < 0 || device >= nd || device >= 64) return ORBX_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return ORBX_ERR_HIP;
  RansacDevice& d = devs[device];
  std::call_once(d.once, [&] {
    d.init_err = hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking);
    if (d.init_err == hipSuccess && kernel_setup) d.init_err = kernel_setup();
    if (d.init_err == hipSuccess) d.init_err = d.pinned_reserve(1 << 16);
  });
  return d.init_err == hipSuccess ? ORBX_OK : ORBX_ERR_HIP;
}

// H minimal sets of set_size indices out of N: DUtils::Random::RandomInt(0, size-1) on the
// rand() values rv[0 .. H*set_size) plus swap-remove, as the reference's iterate() loops draw them.
inline void ransac_sample_sets(const int32_t* rv, int H, int set_size, int N, int* sets) {
  std::vector<int> avail(N > 0 ? N : 1);
  for (int k = 0; k < H; k++) {
    for (int i = 0; i < N; i++) avail[i] = i;
    int size = N;
    for (int i = 0; i < set_size; i++) {
      const int32_t v = rv[(size_t)k * set_size + i];
      const int randi = (int)(((double)v / ((double)RAND_MAX + 1.0)) * size);
      sets[(size_t)k * set_size + i] = avail[randi];
      avail[randi] = avail[size - 1];
      size--;
    }
  }
}

// The next n values of a copy of the stream (the values a call may consume) ...
inline std::vector<int32_t> rand_peek(const orbx_rand_state* rng, size_t n) {
  orbx_rand_state peek = *rng;
  std::vector<int32_t> vals(n > 0 ? n : 1);
  for (size_t k = 0; k < n; k++) vals[k] = orbx_rand_next(&peek);
  return vals;
}

// ... and the caller's stream moved past the `used` values the call did consume.
inline void rand_advance(orbx_rand_state* rng, size_t used) {
  for (size_t k = 0; k < used; k++) (void)orbx_rand_next(rng);
}

}  // namespace orbx

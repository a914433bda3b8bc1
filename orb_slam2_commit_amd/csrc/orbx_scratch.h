// orbx_scratch.h -- scratch for the per-call host APIs (SearchByBoW, PoseOptimization,
// SearchByProjection, SearchForTriangulation, ComputeDistinctiveDescriptors, UndistortKeyPoints,
// OptimizeSim3 and the debug probes).
//
// The reference calls these once per frame / KeyFrame from the Tracking and LocalMapping threads,
// so each call must not pay a device allocation: hipFree synchronises the whole device (stalling
// every other stream, e.g. the other thread's extraction), and pageable hipMemcpy goes through the
// null stream.  A call instead leases a per-device scratch record -- a grow-only device arena, a
// grow-only pinned host staging block, its own non-blocking stream -- from a pool, and returns it
// when done.  Concurrent callers get different leases (the pool grows to the peak concurrency),
// so calls from different threads still run side by side.  Nothing is freed on the call path;
// the leases live for the process.
//
// Staging is how a host form uses a lease: it declares its arrays as typed slots in the one order
//   inputs | descriptors | outputs | device-only
// (each slot 256-aligned, the same offset in the pinned block and in the device arena), commits,
// fills the descriptor with device addresses, and then moves each side of PCIe in one copy:
// upload() sends the block up to the outputs (or through them, zeroed), download() brings back
// exactly the outputs, fetch() hands them to the caller.  The device-only slots are behind
// everything that is copied and have no pinned bytes.  A slot declared out of that order makes
// commit() fail, so no site can split a transfer in two by accident.
//
// with_stream_block is the device batch forms' counterpart: descriptors (and per-row scratch) in
// one stream-ordered allocation on the caller's stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "../../include/orbx.h"
#include "orbx_mem.h"

namespace orbx {

constexpr size_t scratch_align(size_t x) { return (x + 255) & ~(size_t)255; }
// What a block allocates when a call asks for more bytes than it holds, a quarter of slack each: a lease's
// two blocks, and the LocalBA arenas (ba_host.h Arena; stated here, where a host-only test can reach it).
constexpr size_t lease_capacity(size_t bytes) { return scratch_align(bytes + bytes / 4); }
constexpr size_t arena_capacity(size_t bytes) { return bytes + bytes / 4 + 4096; }
// What a pinned block and its device twin hold together: the smaller of the two capacities (the pinned
// owner rounds up to whole pages, the device owner does not), so growth is decided against this one.
// mapped: there is no twin.
constexpr size_t pair_capacity(size_t pinned_cap, size_t device_cap, bool mapped) {
  return mapped || pinned_cap < device_cap ? pinned_cap : device_cap;
}

// (A lease is a heap object that is never deleted -- see orbx_mem.h on process-lifetime owners.)
struct ScratchLease {
  int device = 0;
  hipStream_t st = nullptr;
  uint8_t* d = nullptr;  // device arena (dmem's block)
  uint8_t* h = nullptr;  // pinned host staging (hmem's block)
  DevBuf<uint8_t> dmem;
  PinnedBuf hmem;
  // grow-only: on growth the old blocks are released first (the lease is idle between calls)
  hipError_t reserve(size_t dbytes, size_t hbytes);
  // wait for the lease's stream (the calls are synchronous, as the reference's are)
  hipError_t sync() { return hipStreamSynchronize(st); }
};

// a lease for the current device (hipSetDevice done by the caller); nullptr on failure
ScratchLease* scratch_acquire(int device);
void scratch_release(ScratchLease* l);

struct ScratchGuard {
  ScratchLease* l;
  explicit ScratchGuard(int device) : l(scratch_acquire(device)) {}
  ~ScratchGuard() {
    if (l) scratch_release(l);
  }
  ScratchGuard(const ScratchGuard&) = delete;
  ScratchGuard& operator=(const ScratchGuard&) = delete;
};

// The device check of every host form: ORBX_ERR_NODEV without a device, ORBX_ERR_ARG for an index
// out of range (or one hipSetDevice refuses).
orbx_status select_device(int device);

class Staging {
 public:
  // `present` is false for a default slot and for an in_opt without a source: dev() gives nullptr
  template <class T>
  struct Slot {
    size_t off = 0, count = 0;
    bool present = false;
  };
  enum class Outputs { zeroed, skipped };  // what upload() does with the output region

  explicit Staging(int device) : device_(device) {}
  ~Staging() { scratch_release(l_); }
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;

  // ---- layout: arithmetic only, in region order
  template <class T>
  Slot<T> in(const T* src, size_t count) {  // (without a source the slot reads as zeros)
    return place<T>(kIn, src, count, true);
  }
  template <class T>
  Slot<T> in_opt(const T* src, size_t count) {
    return place<T>(kIn, src, src ? count : 0, src != nullptr);
  }
  template <class T>
  Slot<T> record(size_t count = 1) {  // filled after commit() (fill), once dev() has addresses
    return place<T>(kRecord, nullptr, count, true);
  }
  template <class T>
  Slot<T> out(size_t count) {
    return place<T>(kOut, nullptr, count, true);
  }
  template <class T>
  Slot<T> inout(const T* src, size_t count) {  // an output with an initial value (zero without src)
    return place<T>(kOut, src, count, true);
  }
  template <class T>
  Slot<T> device_only(size_t count) {
    return place<T>(kDeviceOnly, nullptr, count, true);
  }

  size_t upload_bytes(Outputs m) const { return m == Outputs::zeroed ? outputs_end() : outputs_begin(); }
  size_t outputs_begin() const { return begin(kOut); }
  size_t outputs_end() const { return begin(kDeviceOnly); }
  size_t pinned_bytes() const { return outputs_end(); }
  size_t device_bytes() const { return end_; }

  // ---- the lease.  ORBX_ERR_ARG for a slot out of order; else the lease with both blocks reserved,
  // the pinned output region zeroed and every source copied in (ORBX_ERR_HIP on failure).
  orbx_status commit();
  template <class T>
  T* dev(Slot<T> s) const {
    return s.present ? (T*)(l_->d + s.off) : nullptr;
  }
  template <class T>
  T* host(Slot<T> s) const {
    return (T*)(l_->h + s.off);
  }
  template <class T>
  void fill(Slot<T> s, const T& v, size_t i = 0) {
    std::memcpy(host(s) + i, &v, sizeof(T));
  }
  hipStream_t stream() const { return l_->st; }
  hipError_t upload(Outputs m) { return hipMemcpyAsync(l_->d, l_->h, upload_bytes(m), hipMemcpyHostToDevice, l_->st); }
  hipError_t download() {
    return hipMemcpyAsync(l_->h + outputs_begin(), l_->d + outputs_begin(), outputs_end() - outputs_begin(),
                          hipMemcpyDeviceToHost, l_->st);
  }
  hipError_t sync() { return l_->sync(); }
  template <class T>
  void fetch(Slot<T> s, T* dst, size_t count) const {  // (an output the caller did not ask for: dst null)
    if (dst && count) std::memcpy(dst, host(s), count * sizeof(T));
  }

 private:
  enum { kIn, kRecord, kOut, kDeviceOnly };
  struct Copy {
    const void* src;  // null: zeros
    size_t off, bytes;
  };
  size_t begin(int region) const { return region <= region_ ? begin_[region] : end_; }
  template <class T>
  Slot<T> place(int region, const void* src, size_t count, bool present) {
    if (region < region_) bad_ = true;
    while (region_ < region) begin_[++region_] = end_;
    const Slot<T> s{end_, count, present};
    if (count && (src || region == kIn)) copies_.push_back({src, end_, count * sizeof(T)});
    end_ += scratch_align(count * sizeof(T));
    return s;
  }

  int device_;
  ScratchLease* l_ = nullptr;
  int region_ = kIn;
  size_t begin_[4] = {0, 0, 0, 0}, end_ = 0;
  bool bad_ = false;
  std::vector<Copy> copies_;
};

// bytes of stream-ordered device memory for fn(uint8_t* d) -> hipError_t, which enqueues on `st`;
// freed on `st` whether or not fn succeeded.  ORBX_ERR_HIP if any step failed.
template <class Fn>
orbx_status with_stream_block(size_t bytes, hipStream_t st, Fn&& fn) {
  uint8_t* d = nullptr;
  if (hipMallocAsync((void**)&d, bytes, st) != hipSuccess) return ORBX_ERR_HIP;
  const hipError_t e = fn(d);
  const hipError_t e2 = hipFreeAsync(d, st);
  return e != hipSuccess || e2 != hipSuccess ? ORBX_ERR_HIP : ORBX_OK;
}

}  // namespace orbx

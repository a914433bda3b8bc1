// orbx_mem.h -- the owners of device and pinned memory, of events and of streams: every handle in
// csrc/ holds its blocks through these, so no destroy function keeps a list and no error path unwinds
// by hand.  Host only: no launch, no device code.  hipMalloc / hipFree / hipHostMalloc / hipHostFree
// are called here and nowhere else.
//
// An owner frees in its destructor, so it must not outlive the HIP runtime.  Three kinds of object
// live for the whole process and are therefore reached through pointers that are allocated once and
// never deleted, so nothing of theirs is ever freed: the RANSAC
// solvers' per-device contexts (pnp.hip g_pnp_dev, sim3.hip g_sim3_dev, initializer.hip g_init_dev --
// one `new RansacDevice[64]` each) and the scratch leases of scratch.hip's pool.  An owner with
// static storage would call hipFree / hipHostFree during static destruction, after the runtime may
// be gone; do not add one.
//
// Growth policy is the site's business: ensure() allocates what it is asked for (PinnedBuf rounds
// that up to whole pages) and a site that wants slack passes the padded figure.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace orbx {

// device memory, count elements of T; grow-only through ensure()
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept { swap(o); }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      swap(o);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void swap(DevBuf& o) noexcept {
    std::swap(p, o.p);
    std::swap(n, o.n);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  // a no-op when count <= n; else the old block is freed and max(count, 1) elements allocated (the
  // contents are not kept).  On failure the owner is empty.
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    release();
    const size_t c = std::max<size_t>(count, 1);
    const hipError_t e = hipMalloc((void**)&p, c * sizeof(T));
    if (e == hipSuccess)
      n = c;
    else
      p = nullptr;
    return e;
  }
  hipError_t upload(const T* src, size_t count) {  // a blocking copy of a host table
    const hipError_t e = ensure(count);
    return e != hipSuccess || !count ? e : hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
  }
  hipError_t upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }
};

// what PinnedBuf::ensure(bytes) allocates: whole 4 KiB pages, at least one
constexpr size_t pinned_pages(size_t bytes) { return ((bytes ? bytes : 1) + 4095) & ~(size_t)4095; }

// pinned host bytes; mapped: the device reads and writes the block in place through dev()
struct PinnedBuf {
  uint8_t* p = nullptr;
  size_t cap = 0;
  explicit PinnedBuf(bool mapped = false) : mapped_(mapped) {}
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  PinnedBuf(PinnedBuf&& o) noexcept : mapped_(o.mapped_) { swap(o); }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) {
      release();
      swap(o);
    }
    return *this;
  }
  ~PinnedBuf() { release(); }
  void swap(PinnedBuf& o) noexcept {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    std::swap(d_, o.d_);
    std::swap(mapped_, o.mapped_);
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = d_ = nullptr;
    cap = 0;
  }
  bool mapped() const { return mapped_; }
  // a no-op when bytes <= cap; else the old block is freed and pinned_pages(bytes) allocated (the
  // contents are not kept).  On failure the owner is empty.
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    release();
    const size_t c = pinned_pages(bytes);
    hipError_t e = hipHostMalloc((void**)&p, c, mapped_ ? hipHostMallocMapped : hipHostMallocDefault);
    if (e != hipSuccess) p = nullptr;
    if (e == hipSuccess && mapped_) e = hipHostGetDevicePointer((void**)&d_, p, 0);
    if (e == hipSuccess)
      cap = c;
    else
      release();
    return e;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
  // the device's view of a mapped block (nullptr when empty or not mapped)
  template <class T = uint8_t>
  T* dev() const {
    return reinterpret_cast<T*>(d_);
  }

 private:
  uint8_t* d_ = nullptr;
  bool mapped_;
};

// an event, created on first use
struct Event {
  hipEvent_t ev = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (ev) (void)hipEventDestroy(ev);
  }
  hipError_t ensure(unsigned flags = hipEventDisableTiming) {
    return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags);
  }
  operator hipEvent_t() const { return ev; }
};

// a non-blocking stream a handle owns
struct Stream {
  hipStream_t st = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (st) (void)hipStreamDestroy(st);
  }
  hipError_t ensure() { return st ? hipSuccess : hipStreamCreateWithFlags(&st, hipStreamNonBlocking); }
  operator hipStream_t() const { return st; }
};

}  // namespace orbx

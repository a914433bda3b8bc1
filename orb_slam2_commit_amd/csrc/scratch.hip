// scratch.hip -- the per-device lease pool of orbx_scratch.h.
#include <mutex>
#include <vector>

#include "orbx_scratch.h"

namespace orbx {

namespace {
struct Pool {
  std::mutex mu;
  std::vector<ScratchLease*> free;
};
constexpr int kMaxDevices = 64;
Pool g_pool[kMaxDevices];
}  // namespace

hipError_t ScratchLease::reserve(size_t dbytes, size_t hbytes) {
  dbytes = dbytes ? dbytes : 256;
  hbytes = hbytes ? hbytes : 256;
  if (dbytes > dmem.n) {
    if (d) {
      hipError_t e = hipStreamSynchronize(st);  // the previous call's work is done (defensive)
      if (e != hipSuccess) return e;
    }
    const hipError_t e = dmem.ensure(lease_capacity(dbytes));
    d = dmem.p;
    if (e != hipSuccess) return e;
  }
  if (hbytes > hmem.cap) {
    const hipError_t e = hmem.ensure(lease_capacity(hbytes));
    h = hmem.p;
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

ScratchLease* scratch_acquire(int device) {
  if (device < 0 || device >= kMaxDevices) return nullptr;
  Pool& p = g_pool[device];
  {
    std::lock_guard<std::mutex> lock(p.mu);
    if (!p.free.empty()) {
      ScratchLease* l = p.free.back();
      p.free.pop_back();
      return l;
    }
  }
  ScratchLease* l = new (std::nothrow) ScratchLease();
  if (!l) return nullptr;
  l->device = device;
  if (hipStreamCreateWithFlags(&l->st, hipStreamNonBlocking) != hipSuccess) {
    delete l;
    return nullptr;
  }
  return l;
}

void scratch_release(ScratchLease* l) {
  if (!l) return;
  Pool& p = g_pool[l->device];
  std::lock_guard<std::mutex> lock(p.mu);
  p.free.push_back(l);
}

orbx_status select_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ORBX_ERR_NODEV;
  if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return ORBX_ERR_ARG;
  return ORBX_OK;
}

orbx_status Staging::commit() {
  if (bad_) return ORBX_ERR_ARG;
  if (!l_) l_ = scratch_acquire(device_);
  if (!l_ || l_->reserve(device_bytes(), pinned_bytes()) != hipSuccess) return ORBX_ERR_HIP;
  std::memset(l_->h + outputs_begin(), 0, outputs_end() - outputs_begin());
  for (const Copy& c : copies_) {
    if (c.src)
      std::memcpy(l_->h + c.off, c.src, c.bytes);
    else
      std::memset(l_->h + c.off, 0, c.bytes);
  }
  return ORBX_OK;
}

}  // namespace orbx

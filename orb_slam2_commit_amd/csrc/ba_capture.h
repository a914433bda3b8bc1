// ba_capture.h -- LocalBundleAdjustment (localba.hip): the test-only capture of one LM trial's
// linear algebra (include/orbx_debug.h, orbx_debug_ba_capture_select / _read).  Two kernels that
// only copy: k_ba_capture_pre between k_ba_schur_fin and the LDLT (the state the errors were
// computed at, the structure, S and bs before the factorisation overwrites them, lambda and chi),
// k_ba_capture_post after k_ba_update (the solve's xp, the pushed state cbak / Xbak and the point
// step).  optimize_dev launches them only while a capture is selected for the running phase; the
// device LM state picks the trial, like the other gated kernels.  (Included by ba_host.h after its
// HIP_TRY, which the host half below uses.)
#pragma once
#include "ba_lm.h"

namespace orbx {

constexpr int kCapHdr = 8;  // hdr: fired, it, qmax, solve ok, armed, trial (LmState::trials at the trial's start)

struct BaCapDev {
  int* hdr;
  double* sc;  // lambda, currentChi
  double *cq, *ct, *X, *eerr, *S, *bs;     // k_ba_capture_pre
  double *xp, *cbak, *Xbak, *xl;           // k_ba_capture_post
  int *act, *pose_cam, *pt_id, *erobust;   // k_ba_capture_pre
  int sel_it, sel_q;
};

template <class T, class U>
__device__ inline void cap_copy(T* dst, const U* src, size_t n) {
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) dst[i] = (T)src[i];
}

// hdr[0] (fired) is written by k_ba_capture_post alone and read here alone; hdr[4], hdr[5] are written
// here (one thread) and read by the post kernel: no word is read and written in the same launch.
__global__ __launch_bounds__(LBS) void k_ba_capture_pre(BaDev D, BaCapDev C) {
  const LmState* L = D.lm;
  if (L->done || C.hdr[0] != 0 || (C.sel_it >= 0 && L->it != C.sel_it) || L->qmax != C.sel_q) return;
  const size_t N = 6 * (size_t)D.nposes;
  cap_copy(C.cq, D.cq, 4 * (size_t)D.nc);
  cap_copy(C.ct, D.ct, 3 * (size_t)D.nc);
  cap_copy(C.X, D.X, 3 * (size_t)D.np);
  cap_copy(C.eerr, D.eerr, 3 * (size_t)D.ne);
  cap_copy(C.erobust, D.erobust, (size_t)D.ne);
  cap_copy(C.act, D.act, (size_t)D.na);
  cap_copy(C.pt_id, D.pt_id, (size_t)D.npa);
  cap_copy(C.pose_cam, D.pose_cam, (size_t)D.nposes);
  cap_copy(C.S, D.S, N * N);
  cap_copy(C.bs, D.bs, N);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    C.hdr[1] = L->it;
    C.hdr[2] = L->qmax;
    C.hdr[5] = L->trials;
    C.hdr[4] = 1;
    C.sc[0] = L->lambda;
    C.sc[1] = L->currentChi;
  }
}

__global__ __launch_bounds__(LBS) void k_ba_capture_post(BaDev D, BaCapDev C) {
  if (C.hdr[4] != 1 || C.hdr[5] != D.lm->trials) return;  // not the trial k_ba_capture_pre took
  const bool ok = D.scal[2] != 0.0;
  if (ok) {  // (a failed solve pushes nothing: the items stay zero)
    const size_t step = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    cap_copy(C.xp, D.xp, 6 * (size_t)D.nposes);
    for (size_t i = i0; i < 7 * (size_t)D.nposes; i += step) C.cbak[i] = D.cbak[7 * (size_t)D.pose_cam[i / 7] + i % 7];
    for (size_t i = i0; i < 3 * (size_t)D.npa; i += step) {
      const size_t s = 3 * (size_t)D.pt_id[i / 3] + i % 3;
      const double b = D.Xbak[s];
      C.Xbak[i] = b;
      C.xl[i] = D.X[s] - b;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    C.hdr[3] = ok ? 1 : 0;
    C.hdr[0] = 1;
  }
}

// Host side of the capture (a member of LocalBA): the selection, the device buffers and the host copy
// orbx_debug_ba_capture_read serves.
struct BaCapture {
  int sel_phase = -1, sel_it = -1, sel_q = 0;  // sel_phase < 0: off
  int cur_phase = 0;                           // the phase optimize_dev is running (run_local_ba sets it)
  DevBuf<double> dd;
  DevBuf<int> di;
  std::vector<double> hd;
  std::vector<int> hi;
  int dims[7] = {0, 0, 0, 0, 0, 0, 0};  // phase, nc, np, ne, na, npa, nposes of the host copy
  bool have = false;

  bool on() const { return sel_phase >= 0 && sel_phase == cur_phase; }
  // item `what` (ORBX_BA_CAP_*, HEADER excepted) of a capture with these sizes: offset and count in
  // the double (is_int = false) or the int buffer
  static bool item(int what, const int d[7], bool* is_int, size_t* off, size_t* cnt) {
    const size_t nc = d[1], np = d[2], ne = d[3], na = d[4], npa = d[5], N = 6 * (size_t)d[6];
    const size_t nd[] = {2, 4 * nc, 3 * nc, 3 * np, 3 * ne, N * N, N, N, 7 * (size_t)d[6], 3 * npa, 3 * npa};
    const size_t ni[] = {na, (size_t)d[6], npa, ne};
    if (what >= ORBX_BA_CAP_LAMBDA_CHI && what <= ORBX_BA_CAP_XL) {
      *is_int = false;
      *off = 0;
      for (int i = 0; i < what - ORBX_BA_CAP_LAMBDA_CHI; i++) *off += nd[i];
      *cnt = nd[what - ORBX_BA_CAP_LAMBDA_CHI];
      return true;
    }
    if (what >= ORBX_BA_CAP_ACT && what <= ORBX_BA_CAP_EROBUST) {
      *is_int = true;
      *off = kCapHdr;
      for (int i = 0; i < what - ORBX_BA_CAP_ACT; i++) *off += ni[i];
      *cnt = ni[what - ORBX_BA_CAP_ACT];
      return true;
    }
    return false;
  }
  static void totals(const int d[7], size_t* nd, size_t* ni) {
    bool b;
    size_t o, c;
    item(ORBX_BA_CAP_XL, d, &b, &o, &c);
    *nd = o + c;
    item(ORBX_BA_CAP_EROBUST, d, &b, &o, &c);
    *ni = o + c;
  }
  // a phase with a capture selected begins: zeroed device buffers for these sizes
  hipError_t begin(const BaDev& D, BaCapDev* C, hipStream_t st) {
    have = false;
    const int d[7] = {cur_phase, D.nc, D.np, D.ne, D.na, D.npa, D.nposes};
    std::memcpy(dims, d, sizeof d);
    size_t nd, ni;
    totals(dims, &nd, &ni);
    HIP_TRY(dd.ensure(nd));
    HIP_TRY(di.ensure(ni));
    HIP_TRY(hipMemsetAsync(dd.p, 0, nd * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(di.p, 0, ni * sizeof(int), st));
    auto pd = [&](int what) {
      bool b;
      size_t o, c;
      item(what, dims, &b, &o, &c);
      return dd.p + o;
    };
    auto pi = [&](int what) {
      bool b;
      size_t o, c;
      item(what, dims, &b, &o, &c);
      return di.p + o;
    };
    C->hdr = di.p;
    C->sc = pd(ORBX_BA_CAP_LAMBDA_CHI);
    C->cq = pd(ORBX_BA_CAP_CQ);
    C->ct = pd(ORBX_BA_CAP_CT);
    C->X = pd(ORBX_BA_CAP_X);
    C->eerr = pd(ORBX_BA_CAP_EERR);
    C->S = pd(ORBX_BA_CAP_S);
    C->bs = pd(ORBX_BA_CAP_BS);
    C->xp = pd(ORBX_BA_CAP_XP);
    C->cbak = pd(ORBX_BA_CAP_CBAK);
    C->Xbak = pd(ORBX_BA_CAP_XBAK);
    C->xl = pd(ORBX_BA_CAP_XL);
    C->act = pi(ORBX_BA_CAP_ACT);
    C->pose_cam = pi(ORBX_BA_CAP_POSE_CAM);
    C->pt_id = pi(ORBX_BA_CAP_PT_ID);
    C->erobust = pi(ORBX_BA_CAP_EROBUST);
    C->sel_it = sel_it;
    C->sel_q = sel_q;
    return hipSuccess;
  }
  static int grid(const BaDev& D) {
    const size_t N = 6 * (size_t)D.nposes;
    const size_t m = std::max({N * N, 3 * (size_t)D.ne, 4 * (size_t)D.nc, 3 * (size_t)D.np, (size_t)1});
    return (int)std::min<size_t>((m + LBS - 1) / LBS, 256);
  }
  // the phase has ended and the stream is idle: the host copy
  hipError_t end() {
    size_t nd, ni;
    totals(dims, &nd, &ni);
    hd.resize(nd);
    hi.resize(ni);
    HIP_TRY(hipMemcpy(hd.data(), dd.p, nd * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hi.data(), di.p, ni * sizeof(int), hipMemcpyDeviceToHost));
    have = true;
    return hipSuccess;
  }
};

}  // namespace orbx

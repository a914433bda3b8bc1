// ba_host.h -- LocalBundleAdjustment (localba.hip): the host object of one solver.  Device buffers
// and arenas, the phase structure (host and device builds), and the device-LM driver of one
// optimize() call (LocalBA::optimize_dev), with the stop-flag mirror it polls.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <limits>
#include <thread>
#include <vector>

#include "ba_ldlt.h"
#include "ba_lm.h"
#include "ba_schur.h"
#include "ba_structure.h"
#include "orbx_scratch.h"

namespace orbx {

// ------------------------------------------------------------------ host

struct Ctx {
  DevBuf<double> cbak, Xbak, eerr, Hpl, ptc, cmc, BD, cf, Hll, bl, Dinv, dmax_p, Hpp, bp, xp, bs, S, Sw, scal, gpart, gpose;

  DevBuf<int> ptab;
  DevBuf<uint8_t> flag;
  DevBuf<LmState> lm;
  DevBuf<uint8_t> prob;  // k_ba_prep outputs: FP64 points and edge arrays
};

#define HIP_TRY(x)                      \
  do {                                  \
    const hipError_t e_ = (x);          \
    if (e_ != hipSuccess) return e_;    \
  } while (0)
#define BA_CHECK(x)                          \
  do {                                       \
    if ((x) != hipSuccess) return ORBX_ERR_HIP; \
  } while (0)

// A pinned host block and its device twin, carved by take() in the same offsets: arrays are laid
// out with take(), filled through host(), and sent with one async copy (upload).  mapped: no
// twin -- dbuf() is the device's view of the pinned block itself, so kernels write results straight
// into host memory (no copy, no copy engine hand-off after the last kernel)
// (grows to arena_capacity(bytes), orbx_scratch.h)
struct Arena {
  PinnedBuf hmem;
  DevBuf<uint8_t> dmem;  // the twin (empty when mapped)
  size_t off = 0;
  const bool mapped;
  explicit Arena(bool m = false) : hmem(m), mapped(m) {}
  uint8_t* hbuf() const { return hmem.p; }
  uint8_t* dbuf() const { return mapped ? hmem.dev() : dmem.p; }  // the device's side of the block
  // what take() may hand out: the smaller side (the pinned owner rounds up to pages, the twin does not)
  size_t capacity() const { return pair_capacity(hmem.cap, dmem.n, mapped); }
  // both sides hold at least `bytes`, or neither holds anything
  hipError_t reserve(size_t bytes) {
    off = 0;
    if (bytes <= capacity() && hbuf() && dbuf()) return hipSuccess;
    const size_t cap = arena_capacity(bytes);
    hipError_t e = hmem.ensure(cap);
    if (e == hipSuccess && !mapped) e = dmem.ensure(cap);
    if (e != hipSuccess) {
      hmem.release();
      dmem.release();
    }
    return e;
  }
  template <class T>
  T* take(size_t n) {
    off = scratch_align(off);
    T* d = reinterpret_cast<T*>(dbuf() + off);
    off += std::max<size_t>(n, 1) * sizeof(T);
    return d;
  }
  template <class T>
  T* host(T* d) {
    return reinterpret_cast<T*>(hbuf() + (reinterpret_cast<uint8_t*>(d) - dbuf()));
  }
  template <class T>
  T* put(const std::vector<T>& v) {
    T* d = take<T>(v.size());
    if (!v.empty()) std::memcpy(host(d), v.data(), v.size() * sizeof(T));
    return d;
  }
  hipError_t upload(hipStream_t st) {
    return off && !mapped ? hipMemcpyAsync(dbuf(), hbuf(), off, hipMemcpyHostToDevice, st) : hipSuccess;
  }
};

inline size_t arena_bytes(std::initializer_list<size_t> sizes) {
  size_t t = 0;
  for (size_t x : sizes) t += scratch_align(std::max<size_t>(x, 1));
  return t + 256;
}

}  // namespace orbx
#include "ba_capture.h"  // (uses HIP_TRY above)
namespace orbx {

struct LocalBA {
  BaDev D{};
  BaCapture cap;  // test-only capture of one trial (orbx_debug_ba_capture_select); off by default
  Ctx c;  // device buffers, kept across calls (grow only)
  Arena prob_arena, struct_arena;
  // result write-back: k_ba_outliers / k_ba_export write the flags, poses and points straight
  // into a mapped pinned block, then host copies into the caller's arrays.  (A device arena read
  // back by one copy measured 81 us of copy-engine hand-off after k_ba_export plus the 11 us copy
  // per call, profiles/r05/localba_timeline_*.txt)
  Arena wb_arena{true};
  struct Wb {
    double *Tcw_d, *Xw_d;
    float *Tcw, *Xw;
    uint8_t* flag;
  } wb{};
  std::vector<int> e_pt, e_cam;
  std::vector<uint8_t> fixed;
  std::vector<uint8_t> level;  // 0/1 per edge
  int trials = 0;
  int nbu = 1, n_rb = 8;           // k_ba_update blocks; doubles in the readback block
  PinnedBuf rb{true};              // pinned readback block, n_rb doubles (mapped: kernels write it in place)
  Event rb_ev;                     // recorded after the readback copy (the wait skips later work)
  // the linearisation outputs the LM trials read
  struct LinSet {
    double *Hpl, *Hll, *bl, *dmax_p, *Hpp, *bp;
  };
  LinSet lin0 = {};
  LocalBA() = default;
  LocalBA(const LocalBA&) = delete;
  LocalBA& operator=(const LocalBA&) = delete;
  PinnedBuf own_stop{true};  // orbx_ba_stop_flag: one int, pinned, device-readable
  bool hook_stopped = false;  // ORBX_BA_RAISE_STOP_AFTER fired (the host then stops as for a raised flag)
  static void use_lin(BaDev& D, const LinSet& L) {
    D.Hpl = L.Hpl;
    D.Hll = L.Hll;
    D.bl = L.bl;
    D.Hpp = L.Hpp;
    D.bp = L.bp;
    D.dmax_p = L.dmax_p;
    D.dmax_c = L.dmax_p + D.npa;  // contiguous: one max-reduction for lambda init
  }
  // computeActiveErrors is not repeated: the errors/chi stored by the trial
  // (recompute, slot 1) are the ones at the state being linearised
  static void lin_points(const BaDev& Dl, hipStream_t st) {
    const int ga = std::max((Dl.na + LBS - 1) / LBS, 1);
    if (Dl.na > 0) hipLaunchKernelGGL(k_ba_linearize, dim3(ga), dim3(LBS), 0, st, Dl);
    if (Dl.npa > 0) hipLaunchKernelGGL(k_ba_point_sum, dim3((Dl.npa + LBS - 1) / LBS), dim3(LBS), 0, st, Dl);
  }
  // fused point side (k_ba_lin_schur): edges grouped by point with at most kFuseMaxDeg per point
  bool fuse_ok = false;
  DevBuf<int> pblk;
  // host scratch, reused across calls
  std::vector<int> act, pos_pt, chidx, pose_cam, pt_off, pt_id, cam_off, cam_pos, cnt, pcam, ccnt, ccnt4, boff;

  // Active set of a phase: SparseOptimizer::initializeOptimization(level) +
  // buildIndexMapping; point-major positions, pose groups (positions
  // ascending within each pose).  Edges arriving grouped by point (the
  // reference adds them per MapPoint, Optimizer.cc:659-745) take the one-pass
  // path; otherwise a stable counting sort by point.  Schur pairs are found on
  // the device (k_ba_pairs), not listed here.
  double t_struct[4] = {0, 0, 0, 0};  // host ms: index/CSR, pose groups, device build, upload+alloc
  bool dev_struct = false;  // k_ba_struct_* build the arrays (edges grouped by point, nc <= kStructMaxNc)
  const uint8_t* dfix = nullptr;  // device copy of the fixed flags
  DevBuf<int> sbuf;               // k_ba_struct_* tiles and outputs, sized for the whole edge list
  PinnedBuf sint{true};           // pinned, mapped: k_ba_struct_scan's five sizes (written there directly)
  int sizes1[5] = {0, 0, 0, 0, 0};  // phase-1 sizes (all edges active), counted on the host
  orbx_status build_structure(int lvl, hipStream_t st) {
    if (dev_struct) return build_structure_dev(lvl, st, lvl < 0 ? sizes1 : nullptr);
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
      return std::chrono::duration<double, std::milli>(b - a).count();
    };
    const auto T0 = now();
    const int nc = D.nc, np = D.np, ne = D.ne;
    const uint8_t* lv = level.data();
    ccnt.assign(nc, 0);
    int na = 0;
    bool sorted = true;
    for (int e = 0, last = -1; e < ne; e++)
      if (lvl < 0 || lv[e] == lvl) {
        ccnt[e_cam[e]]++;
        na++;
        sorted &= e_pt[e] >= last;
        last = e_pt[e];
      }
    chidx.assign(nc, -1);
    pose_cam.clear();
    cam_off.assign(1, 0);
    for (int c = 0; c < nc; c++)
      if (ccnt[c] && !fixed[c]) {
        chidx[c] = (int)pose_cam.size();
        pose_cam.push_back(c);
        cam_off.push_back(cam_off.back() + ccnt[c]);
      }
    const int nposes = (int)pose_cam.size();
    int maxc = 0;
    for (int ci = 0; ci < nposes; ci++) maxc = std::max(maxc, cam_off[ci + 1] - cam_off[ci]);
    act.resize(na);
    pos_pt.resize(na);
    pcam.resize(na);
    pt_off.clear();
    pt_id.clear();
    if (sorted) {
      int k = 0;
      for (int e = 0; e < ne; e++)
        if (lvl < 0 || lv[e] == lvl) {
          const int p = e_pt[e];
          if (pt_id.empty() || pt_id.back() != p) {
            pt_off.push_back(k);
            pt_id.push_back(p);
          }
          act[k] = e;
          pos_pt[k] = (int)pt_id.size() - 1;
          pcam[k] = chidx[e_cam[e]];
          k++;
        }
      pt_off.push_back(na);
    } else {
      cnt.assign(np + 1, 0);
      for (int e = 0; e < ne; e++)
        if (lvl < 0 || lv[e] == lvl) cnt[e_pt[e] + 1]++;
      pt_off.push_back(0);
      for (int p = 0; p < np; p++) {
        const int n = cnt[p + 1];
        cnt[p + 1] = cnt[p] + n;  // start of point p's positions
        if (n) {
          pt_id.push_back(p);
          pt_off.push_back(cnt[p + 1]);
        }
      }
      for (int e = 0; e < ne; e++)
        if (lvl < 0 || lv[e] == lvl) act[cnt[e_pt[e]]++] = e;  // stable: ascending edge order per point
      for (int i = 0; i < (int)pt_id.size(); i++)
        for (int k = pt_off[i]; k < pt_off[i + 1]; k++) pos_pt[k] = i;
      for (int k = 0; k < na; k++) pcam[k] = chidx[e_cam[act[k]]];
    }
    const int npa = (int)pt_id.size();
    const auto T1 = now();
    cam_pos.resize(cam_off[nposes]);
    {
      std::vector<int>& fill = cnt;  // reuse
      fill.assign(cam_off.begin(), cam_off.end());
      for (int k = 0; k < na; k++)
        if (pcam[k] >= 0) cam_pos[fill[pcam[k]]++] = k;
    }
    const auto T2 = now();
    const auto T3 = T2;
    if (nposes > kTiledMaxPoses) return ORBX_ERR_SIZE;  // before the quadratic tables below
    long long nslots64 = 0;
    for (int c1 = 0; c1 < nposes; c1++) nslots64 += (long long)(cam_off[c1 + 1] - cam_off[c1]) * (nposes - c1);
    if (nslots64 > std::numeric_limits<int>::max()) return ORBX_ERR_SIZE;
    boff.assign(1, 0);
    for (int c1 = 0; c1 < nposes; c1++)
      for (int c2 = c1; c2 < nposes; c2++) boff.push_back(boff.back() + cam_off[c1 + 1] - cam_off[c1]);
    // one upload
    hipError_t he = struct_arena.reserve(arena_bytes({4 * (size_t)na, 4 * (size_t)na, 4 * (size_t)nc,
                                                      4 * (size_t)nposes, 4 * (size_t)(npa + 1), 4 * (size_t)npa,
                                                      4 * (size_t)(nposes + 1), 4 * cam_pos.size(), 4 * (size_t)na,
                                                      4 * boff.size()}));
    if (he != hipSuccess) return ORBX_ERR_HIP;
    Arena& A = struct_arena;
    D.act = A.put(act);
    D.pos_pt = A.put(pos_pt);
    D.chidx = A.put(chidx);
    D.pose_cam = A.put(pose_cam);
    D.pt_off = A.put(pt_off);
    D.pt_id = A.put(pt_id);
    D.cam_off = A.put(cam_off);
    D.cam_pos = A.put(cam_pos);
    D.pcam = A.put(pcam);
    D.boff = A.put(boff);
    BA_CHECK(A.upload(st));
    const orbx_status fs = finish_structure(na, npa, nposes, maxc, boff.back(), st);
    const auto T4 = now();
    t_struct[0] += ms(T0, T1);
    t_struct[1] += ms(T1, T2);
    t_struct[2] += ms(T2, T3);
    t_struct[3] += ms(T3, T4);
    return fs;
  }

  // The same arrays built by k_ba_struct_* from the device-resident edge list
  // and phase flags (no host copy of the flags, no upload); one readback of
  // the five sizes the launch grids and allocations need (none when the
  // sizes are known: phase 1, every edge active).
  orbx_status build_structure_dev(int lvl, hipStream_t st, const int* known) {
    const auto T0 = std::chrono::steady_clock::now();
    BA_CHECK(launch_structure_dev(lvl, st, known, nullptr));
    const int* sz = known;
    if (!sz) {
      BA_CHECK(hipStreamSynchronize(st));
      sz = sint.as<int>();
    }
    const orbx_status fs = finish_structure(sz[0], sz[1], sz[2], sz[3], sz[4], st);
    t_struct[2] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
    return fs;
  }
  // The structure kernels alone (sizes to the mapped sint block unless known); gate: the device LM
  // state that gates them (spec_skip), or null.  The host reads the sizes after the stream's next
  // synchronisation point and calls finish_structure.
  hipError_t launch_structure_dev(int lvl, hipStream_t st, const int* known, const LmState* gate) {
    const int nc = D.nc, ne = D.ne;
    const int ntiles = (ne + kTileE - 1) / kTileE;
    const size_t nb = (size_t)nc * (nc + 1) / 2 + 1;
    HIP_TRY(sbuf.ensure(8 * (size_t)ntiles + (size_t)ntiles * nc + 6 * (size_t)ne + 1 + 3 * (size_t)nc + 1 + nb + 8));
    HIP_TRY(sint.ensure(8 * sizeof(int)));
    int* p = sbuf.p;
    int4* ttot = reinterpret_cast<int4*>(p);  // first: 16-byte aligned
    p += 4 * (size_t)ntiles;
    int4* tcar = reinterpret_cast<int4*>(p);
    p += 4 * (size_t)ntiles;
    int* tcnt = p;
    p += (size_t)ntiles * nc;
    D.act = p, p += ne;
    D.pos_pt = p, p += ne;
    D.pcam = p, p += ne;
    D.cam_pos = p, p += ne;
    D.pt_id = p, p += ne;
    D.pt_off = p, p += ne + 1;
    D.chidx = p, p += nc;
    D.pose_cam = p, p += nc;
    D.cam_off = p, p += nc + 1;
    D.boff = p, p += nb;
    const uint8_t* fl = lvl < 0 ? nullptr : (const uint8_t*)c.flag.p;
    BaDev Ds = D;
    Ds.lm = gate;
    if (ntiles > 0)
      hipLaunchKernelGGL(k_ba_struct_count, dim3(ntiles), dim3(kTileT), sizeof(int) * (nc + kTileT / 64), st, Ds, fl,
                         lvl, tcnt, ttot);
    hipLaunchKernelGGL(k_ba_struct_scan, dim3(1), dim3(kStructNT), sizeof(int) * (nc + 1 + kStructNT / 64), st, Ds,
                       dfix, ntiles, tcnt, ttot, tcar, known ? p : sint.dev<int>());
    if (ntiles > 0)
      hipLaunchKernelGGL(k_ba_struct_fill, dim3(ntiles), dim3(kTileT),
                         sizeof(int) * ((1 + kTileT / 64) * (size_t)nc + kTileE + kTileT / 64), st, Ds, fl, lvl, tcnt,
                         tcar);
    return hipGetLastError();
  }

  // Sizes known: scratch allocations, readback block, Schur pair table.
  orbx_status finish_structure(int na, int npa, int nposes, int maxc, int nslots, hipStream_t st) {
    // the ceiling of the dense reduced system (kTiledMaxN), before any buffer is sized; nslots < 0: the
    // pair table's slot count left the int range (ba_intake, build_structure)
    if (nposes > kTiledMaxPoses || nslots < 0) return ORBX_ERR_SIZE;
    const int gsplit = std::min(std::max((maxc + kGPpt * kGB - 1) / (kGPpt * kGB), 1), 64);
    const size_t N = 6 * (size_t)nposes;
    BA_CHECK(c.Hpl.ensure(18 * (size_t)na));
    BA_CHECK(c.ptc.ensure(12 * (size_t)na));
    BA_CHECK(c.cmc.ensure(kCmc * (size_t)na));
    BA_CHECK(c.BD.ensure(18 * (size_t)na));
    BA_CHECK(c.cf.ensure(6 * (size_t)na));
    BA_CHECK(c.Hll.ensure(9 * (size_t)npa));
    BA_CHECK(c.bl.ensure(3 * (size_t)npa));
    BA_CHECK(c.Dinv.ensure(9 * (size_t)npa));
    BA_CHECK(c.dmax_p.ensure(npa + nposes));
    BA_CHECK(c.Hpp.ensure(36 * (size_t)nposes));
    BA_CHECK(c.bp.ensure(N));
    BA_CHECK(rb_ev.ensure());
    BA_CHECK(c.xp.ensure(N));
    BA_CHECK(c.bs.ensure(N));
    BA_CHECK(c.S.ensure(N * N));
    D.na = na;
    D.npa = npa;
    D.nposes = nposes;
    D.nblk = nposes * (nposes + 1) / 2;
    D.gsplit = gsplit;
    // pairs | rhs | camfold pose terms (64-bit: nblk grows with the square of the poses)
    const size_t ngpart = ((size_t)D.nblk * 36 + (size_t)nposes * 6 + (size_t)nposes * 27) * (size_t)gsplit;
    BA_CHECK(c.gpart.ensure(ngpart));
    D.gpart = c.gpart.p;
    // readback block: scal[0..7], then errors partials (2 slots of nbe), then update partials
    D.nbe = std::max((na + LBS - 1) / LBS, 1);
    nbu = std::max((nposes + LBS - 1) / LBS + (npa + kUpPts - 1) / kUpPts, 1);  // k_ba_update: pose blocks, then point blocks
    D.nbu = nbu;
    n_rb = 8 + 2 * D.nbe + nbu;
    BA_CHECK(c.scal.ensure(n_rb));
    D.scal = c.scal.p;
    BA_CHECK(rb.ensure(n_rb * sizeof(double)));
    BA_CHECK(c.ptab.ensure(nslots));
    D.ptab = c.ptab.p;
    D.nbf = 0;
    D.pblk = nullptr;
    D.fused = 0;  // set on the device-LM copies only
    D.camfold = 0;
    D.posepart = D.bdfold = 0;
    D.gpose = nullptr;
    int npb = 0;  // the pblk blocks, run inside the pair-table launch
    if (fuse_ok && na > 0) {
      D.nbf = (na - 1) / kFuseStride + 1;
      BA_CHECK(pblk.ensure((size_t)D.nbf + 1));
      D.pblk = pblk.p;
      npb = npa / LBS + 1;
      const size_t ng = (size_t)D.nbf * nposes * kCmc;
      if (nposes > 0 && nposes <= kPosePartMaxPoses && ng <= kPosePartMaxDoubles) {
        BA_CHECK(c.gpose.ensure(ng));
        D.gpose = c.gpose.p;
      }
    }
    static_assert(kPB == LBS, "pblk blocks inside k_ba_pair_table");
    if (D.nblk + npb > 0) hipLaunchKernelGGL(k_ba_pair_table, dim3(D.nblk + npb, gsplit), dim3(kPB), 0, st, D);
    BA_CHECK(hipGetLastError());
    D.ptc = c.ptc.p;
    D.cmc = c.cmc.p;
    D.BD = c.BD.p;
    D.cf = c.cf.p;
    D.Dinv = c.Dinv.p;
    D.xp = c.xp.p;
    D.bs = c.bs.p;
    D.S = c.S.p;
    lin0 = LinSet{c.Hpl.p, c.Hll.p, c.bl.p, c.dmax_p.p, c.Hpp.p, c.bp.p};
    use_lin(D, lin0);
    return ORBX_OK;
  }

  hipError_t errors(hipStream_t st, int recompute, int dst) {
    hipLaunchKernelGGL(k_ba_errors, dim3(std::max((D.na + LBS - 1) / LBS, 1)), dim3(LBS), 0, st, D, recompute, dst);
    return hipGetLastError();
  }

  // One readback: out[2] ok flag, out[3] lambda-init max; out[0], out[1]
  // (chi of the two error slots) and out[4] (LM scale) are the block
  // partials added in block order.
  hipError_t read_scalars(double out[5], hipStream_t st) {
    hipError_t e = start_read(st);
    return e == hipSuccess ? finish_read(out) : e;
  }
  hipError_t start_read(hipStream_t st) {
    hipError_t e = hipMemcpyAsync(rb.p, D.scal, n_rb * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(rb_ev, st);
    return e;
  }
  hipError_t finish_read(double out[5]) {
    hipError_t e = wait_event(rb_ev);
    if (e != hipSuccess) return e;
    const double* r = rb.as<double>();
    out[2] = r[2];
    out[3] = r[3];
    const double* p = r + 8;
    double a = 0, b = 0, u = 0;
    for (int i = 0; i < D.nbe; i++) a += p[i];
    for (int i = 0; i < D.nbe; i++) b += p[D.nbe + i];
    for (int i = 0; i < nbu; i++) u += p[2 * D.nbe + i];
    out[0] = a;
    out[1] = b;
    out[4] = u;
    return hipSuccess;
  }

  // SparseOptimizer::optimize + OptimizationAlgorithmLevenberg::solve with the LM control on the
  // device: the entry linearisation and lambda init, then trials queued back to back --
  // (gated) linearisation, Schur, solve, update (which first pops a rejected
  // trial), errors, k_ba_lm_control -- with no host round trip between them,
  // and one gated restore when the phase ends on a rejection.  The host
  // queues as many trials as iterations remain (every trial ends at most one
  // iteration), reads the state back once, and queues more only after
  // rejections; a finished phase turns the queued rest into empty launches.
  PinnedBuf lm_pin{true};      // one LmState, pinned, mapped: the last launch of a batch of trials writes it
  LmState* lm_host() const { return lm_pin.as<LmState>(); }
  // spec (optional): launches queued behind every readback of the phase (before its event), gated on
  // the device LM state (spec_skip) -- phase 1 queues phase 2's outlier marking and structure there
  orbx_status optimize_dev(int iterations, const StopFlag& stop, const DevStop& dstop, hipStream_t st, int* iters,
                           double* final_chi, const std::function<hipError_t()>& spec = nullptr) {
    if (D.nposes > kTiledMaxPoses) return ORBX_ERR_SIZE;  // (finish_structure refuses it before any buffer is sized)
    const size_t N = 6 * (size_t)D.nposes;
    if (!LdltPlan::use_tiled((int)N) && ldlt_np((int)N) > kLdltMaxNp) return ORBX_ERR_SIZE;  // a forced kernel
    LdltPlan ldlt;
    BA_CHECK(ldlt.prepare((int)N));
    D.ldlt_pan = ldlt.pan ? 1 : 0;
    if (ldlt.sw_doubles() > 0) {
      BA_CHECK(c.Sw.ensure(ldlt.sw_doubles()));
      D.Sw = c.Sw.p;
    }
    BA_CHECK(c.lm.ensure(1));
    BA_CHECK(lm_pin.ensure(sizeof(LmState)));
    const int gp = std::max((D.npa + D.nposes + LBS - 1) / LBS, 1);
    const int ga = std::max((D.na + LBS - 1) / LBS, 1);
    const int ge = std::max((D.na + LBS - 1) / LBS, 1);
    double sc[5] = {0, 0, 0, 0, 0};
    BaDev D0 = D;  // ungated: the entry launches and the final chi
    D0.lm = nullptr;
    BaDev Dg = D;
    Dg.lm = c.lm.p;
    Dg.fused = fused_mode(D.nbf, D.nposes);
    Dg.camfold = 1;
    set_trial_folds(Dg);
    int it = 0;
    if (!(stop())) {  // the loop head's first poll (i = 0)
      const bool fused = Dg.nbf > 0;
      // test-only capture of one trial: its two copy kernels are launched only while selected
      const bool capt = cap.on();
      BaCapDev Cd{};
      if (capt) BA_CHECK(cap.begin(D, &Cd, st));
      const int gcap = capt ? BaCapture::grid(D) : 0;
      if (fused) BA_CHECK(set_smem_attr((const void*)k_ba_lin_schur, kFuseSmem));
      // entry: errors, linearisation (point side through k_ba_lin_schur's entry mode when the
      // edges are point-grouped), pose sums, then cam_fin + lambda init + LM init in one launch
      hipLaunchKernelGGL(k_ba_errors, dim3(ge), dim3(LBS), 0, st, D0, 1, 0);
      if (fused) {
        BaDev De = D0;
        De.fused = 3;
        hipLaunchKernelGGL(k_ba_lin_schur, dim3(De.nbf), dim3(kFuseNT), kFuseSmem, st, De);
      } else {
        lin_points(D0, st);
      }
      if (D0.nposes > 0) hipLaunchKernelGGL(k_ba_cam_sum, dim3(D0.nposes, D0.gsplit), dim3(kGB), 0, st, D0);
      hipLaunchKernelGGL(k_ba_lm_start, dim3(1), dim3(1024), 0, st, Dg, iterations);
      BA_CHECK(hipGetLastError());
      const bool psfold = Dg.fused == 2;
      // a trial's errors and LM verdict: two launches by default.  The one-launch form
      // (k_ba_errors_ctl, debug option fused_ctl) pays an agent-scope release per block -- an L2
      // write-back on this multi-XCD part -- and measured 1.5-2.5 % slower per call (profiles/r06)
      const bool split_ctl = ba_opts().fused_ctl == 0;
      auto trial = [&](bool lin) {
        // linearisation gated on the device: only at the start of a new iteration
        if (fused && (lin || psfold)) hipLaunchKernelGGL(k_ba_lin_schur, dim3(Dg.nbf), dim3(kFuseNT), kFuseSmem, st, Dg);
        if (lin && !fused) lin_points(Dg, st);
        // (returns at once after k_ba_lin_schur: the point side of an iteration-start trial is done)
        if (!psfold) hipLaunchKernelGGL(k_ba_point_schur, dim3(ga), dim3(LBS), 0, st, Dg, 0.0);
        if (Dg.nposes > 0) {
          hipLaunchKernelGGL(k_ba_pairs, dim3(Dg.nblk + Dg.nposes, Dg.gsplit), dim3(kPB), 0, st, Dg);
          hipLaunchKernelGGL(k_ba_schur_fin, dim3(Dg.nblk + Dg.nposes), dim3(64), 0, st, Dg, 0.0);
          if (capt) hipLaunchKernelGGL(k_ba_capture_pre, dim3(gcap), dim3(LBS), 0, st, Dg, Cd);
          ldlt.launch(Dg, st);
        } else if (capt) {
          hipLaunchKernelGGL(k_ba_capture_pre, dim3(gcap), dim3(LBS), 0, st, Dg, Cd);
        }
        hipLaunchKernelGGL(k_ba_update, dim3(Dg.nbu), dim3(LBS), 0, st, Dg, 0.0);
        if (capt) hipLaunchKernelGGL(k_ba_capture_post, dim3(gcap), dim3(LBS), 0, st, Dg, Cd);
        if (split_ctl) {
          hipLaunchKernelGGL(k_ba_errors, dim3(ge), dim3(LBS), 0, st, Dg, 1, 1);
          hipLaunchKernelGGL(k_ba_lm_control, dim3(1), dim3(64), 0, st, Dg, dstop);
        } else {
          hipLaunchKernelGGL(k_ba_errors_ctl, dim3(Dg.nbe), dim3(LBS), 0, st, Dg, dstop);
        }
      };
      // (capturing the trial as a HIP graph and launching that instead measured slower on this
      // stack: 2.81 vs 2.76 ms per config-4 call)
      for (int budget = iterations, first = 1;; first = 0) {
        for (int t = 0; t < budget; t++) trial(!(first && t == 0));  // t = 0: linearised by the entry launches
        // the phase's final activeRobustChi2 of the stored errors rides on the same readback
        // (slot 0 is not read by the trials; a batch that did not finish recomputes it later); the
        // launch writes the readback block and the LM state into mapped memory itself
        BaDev Dr = D0;
        Dr.rb_out = rb.dev<double>();
        Dr.lm_out = lm_pin.dev<LmState>();
        Dr.lm_copy = c.lm.p;
        hipLaunchKernelGGL(k_ba_errors, dim3(ge), dim3(LBS), 0, st, Dr, 0, 0);
        BA_CHECK(hipGetLastError());
        if (spec) BA_CHECK(spec());
        BA_CHECK(hipEventRecord(rb_ev, st));
        BA_CHECK(finish_read(sc));
        if (lm_host()->refresh) {  // paused on a NaN-rho rejection: pop, errors at the restored state, resume
          hipLaunchKernelGGL(k_ba_restore, dim3(gp), dim3(LBS), 0, st, Dg);
          hipLaunchKernelGGL(k_ba_errors, dim3(ge), dim3(LBS), 0, st, Dg, 2, 0);
          hipLaunchKernelGGL(k_ba_lm_resume, dim3(1), dim3(64), 0, st, Dg);
          BA_CHECK(hipGetLastError());
        } else if (lm_host()->done) {
          break;
        }
        budget = std::max(1, iterations - lm_host()->it);
      }
      if (capt) BA_CHECK(cap.end());  // (the readback's event has passed: the stream is idle)
      it = lm_host()->it;
      trials += lm_host()->trials;
      hook_stopped |= lm_host()->stopped && D.raise_after >= 0;
      if (lm_host()->rejected) {  // ended on a rejected trial: its pop (chi above reads errors only)
        hipLaunchKernelGGL(k_ba_restore, dim3(gp), dim3(LBS), 0, st, Dg);
        BA_CHECK(hipGetLastError());
      }
    } else {
      hipLaunchKernelGGL(k_ba_errors, dim3(ge), dim3(LBS), 0, st, D0, 0, 0);  // activeRobustChi2 of the stored errors
      BA_CHECK(hipGetLastError());
      BA_CHECK(read_scalars(sc, st));
    }
    *iters = it;
    if (final_chi) *final_chi = sc[0];
    return ORBX_OK;
  }

  // The stop flag as k_ba_lm_control sees it.  The handle's own flag (orbx_ba_stop_flag:
  // pinned, mapped) is read by the device directly.  Any other caller flag is never mapped or
  // registered: the device polls a pinned per-handle MIRROR, and the calling thread -- blocked
  // in the call anyway -- copies the caller's flag into it while it waits for the device
  // (wait_event).  So the device never holds an address whose page the caller may free or
  // remap, and no registration outlives the call (or is shared between handles).
  PinnedBuf mirror{true};  // one int, pinned, mapped
  StopFlag mirror_src;    // the caller flag the mirror follows during a call (empty: none)
  bool map_stop(const StopFlag& s, DevStop* ds) {
    ds->i = nullptr;
    ds->b = nullptr;
    mirror_src = StopFlag{};
    if (!s.i && !s.b) return true;
    if (s.i && own_stop.p && (const void*)s.i == (const void*)own_stop.p) {
      ds->i = own_stop.dev<const int>();
      return true;
    }
    if (mirror.ensure(sizeof(int)) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    mirror_src = s;
    *mirror.as<volatile int>() = s() ? 1 : 0;
    ds->i = mirror.dev<const int>();
    return true;
  }
  void unmap_stop() { mirror_src = StopFlag{}; }
  // hipEventSynchronize that keeps the device's view of the caller's stop flag current
  hipError_t wait_event(hipEvent_t ev) {
    if (!mirror_src.i && !mirror_src.b) return hipEventSynchronize(ev);
    for (;;) {
      const int v = mirror_src() ? 1 : 0;
      if (*mirror.as<volatile int>() != v) *mirror.as<volatile int>() = v;
      const hipError_t q = hipEventQuery(ev);
      if (q != hipErrorNotReady) return q;
      std::this_thread::yield();
    }
  }
};

}  // namespace orbx

// covis.hip -- the covisibility relation as a device-resident observation table: KeyFrame::UpdateConnections
// steps 1-2 (src/KeyFrame.cc:367-467), the vote of Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1523-1581),
// Tracking::UpdateLocalPoints (:1483-1515) and LocalMapping::KeyFrameCulling (src/LocalMapping.cc:784-871, with
// the observation half of KeyFrame::SetBadFlag, src/KeyFrame.cc:585-587, and MapPoint::EraseObservation /
// SetBadFlag, src/MapPoint.cc:113-170), with the reference's exact counts, orders and verdicts.
//
// The table is scanned, not indexed (kfdb.hip's shape): one row per live keyframe in a pool, a feature being
// (point id, octave | stereo | close); per point nObs and bad.  "KF j observes p at idx" is "row j holds p at
// idx" (the contract of include/orbx.h), so no inverse index is stored; a row entry whose point is bad reads
// as -1, which is what EraseMapPointMatch leaves.
//
//   k_covis_row_apply   a row's nObs contributions put in or taken out (integer atomics)
//   k_covis_mark        the query's non-bad points -> bitmap (and back to zero); the vote's bad bytes
//   k_covis_vote        one wave per live keyframe: its row's hits in the bitmap = KFcounter[j]
//   k_covis_commit      the keyframes with a count: id, count, nmax, how many reach th
//   k_covis_rank        place of every such keyframe by id (the counter) and by (weight desc, id desc) among
//                       those >= th (the ordered list); with none, the smallest id among the maxima
//   k_covis_lp_min      per point the smallest (list position << 32 | feature index) over the listed rows
//   k_covis_lp_count    winners (entries owning their point's minimum) per listed keyframe
//   k_covis_lp_emit     winners ranked by key: keyframes before it + prefix inside the row
//   k_covis_cull_*      mark the candidates' points, count / place / fill the per-point observer lists
//   k_covis_cull        ONE workgroup walks the candidates in order, a barrier between them
//   k_covis_compact     moves the live rows to a fresh pool
// Every atomic is an integer add / min / or / max whose result does not depend on arrival order; the only
// arrival-ordered values (positions in the hit list, in a point's observer list, in the went-bad list) are
// ranked by key, walked order-free, or sorted before they leave.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

#include "../../include/orbx.h"
#include "orbx_covis_args.h"
#include "orbx_mem.h"

namespace orbx {

constexpr uint8_t kAuxOct = 0x3f, kAuxStereo = 0x40, kAuxClose = 0x80;  // a pool entry's second byte
constexpr int kCullThreads = 1024;

struct CvMeta {
  long long off;  // first pool entry
  long long id;   // the caller's keyframe id (mnId)
  int32_t len;    // features
  int32_t live;
};

struct CvCtl {
  int n_hit;  // keyframes with a count above zero
  int n_ord;  // of them, those with count >= th
  int nmax;
  int n_win;   // local_points: distinct points
  int total;   // cull: observer-list entries handed out
  int n_bad;   // cull: points that went bad
  int pad[2];
};

struct CvDev {
  const int32_t* pid;
  const uint8_t* aux;
  CvMeta* meta;
  const int32_t* live;
  int n_live;
  int pcap;
  int32_t* nobs;
  uint8_t* bad;
  uint32_t* bitmap;
  unsigned long long* minkey;
  int32_t *pcnt, *pfill, *poff;
  uint32_t* list;
  // per live index
  int32_t* cnt;
  long long* hid;
  int32_t* hw;
  long long* ckf;
  int32_t* cw;
  long long* okf;
  int32_t* ow;
  CvCtl* ctl;
};

// what a vote is taken for: a row of the pool (off = its first entry) or an uploaded list (off = 0)
struct CvSrc {
  const int32_t* ids;
  long long off;
  int n;
  uint8_t* was_bad;  // per entry, or null
};

__device__ __forceinline__ int wave_sum(int v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_covis_row_apply(const int32_t* __restrict__ pid,
                                                         const uint8_t* __restrict__ aux, long long off, int len,
                                                         int32_t* nobs, const uint8_t* __restrict__ bad, int sign) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  const int p = pid[off + i];
  if (p < 0 || bad[p]) return;  // a bad point's nObs is frozen: its observations are gone (src/MapPoint.cc:161)
  atomicAdd(&nobs[p], sign * ((aux[off + i] & kAuxStereo) ? 2 : 1));
}

// mode 0: the source's non-bad points -> bitmap, counters reset; 1: the bitmap back to zero
__global__ __launch_bounds__(256) void k_covis_mark(CvDev D, CvSrc S, int mode) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (mode == 0 && i == 0) {
    D.ctl->n_hit = 0;
    D.ctl->n_ord = 0;
    D.ctl->nmax = 0;
  }
  if (i >= S.n) return;
  const int p = S.ids[S.off + i];
  const bool known = p >= 0 && p < D.pcap;
  if (mode == 1) {
    if (known) D.bitmap[p >> 5] = 0u;
    return;
  }
  const bool isbad = known && D.bad[p];
  if (S.was_bad) S.was_bad[i] = isbad ? 1 : 0;
  if (known && !isbad) atomicOr(&D.bitmap[p >> 5], 1u << (p & 31));
}

// a row's entries whose point is in the bitmap; every lane returns the wave's count
__device__ __forceinline__ int wave_hits(const CvDev& D, const CvMeta& M, int lane) {
  int h = 0;
  for (int base = 0; base < M.len; base += 64) {
    const int i = base + lane;
    bool hit = false;
    if (i < M.len) {
      const int p = D.pid[M.off + i];
      hit = p >= 0 && ((D.bitmap[p >> 5] >> (p & 31)) & 1u);
    }
    h += __popcll(__ballot(hit));
  }
  return h;
}

__global__ __launch_bounds__(256) void k_covis_vote(CvDev D, int self) {
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv >= D.n_live) return;
  const int slot = D.live[wv];
  const CvMeta M = D.meta[slot];
  const int h = wave_hits(D, M, lane);
  if (lane == 0) D.cnt[wv] = slot == self ? 0 : h;  // src/KeyFrame.cc:405: not itself
}

__global__ __launch_bounds__(256) void k_covis_commit(CvDev D, int th) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.n_live) return;
  const int c = D.cnt[i];
  if (c <= 0) return;
  const int pos = atomicAdd(&D.ctl->n_hit, 1);
  D.hid[pos] = D.meta[D.live[i]].id;
  D.hw[pos] = c;
  atomicMax(&D.ctl->nmax, c);
  if (c >= th) atomicAdd(&D.ctl->n_ord, 1);
}

__global__ __launch_bounds__(256) void k_covis_rank(CvDev D, int th) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int m = D.ctl->n_hit;
  if (i >= m) return;
  const int nmax = D.ctl->nmax, n_ord = D.ctl->n_ord;
  const long long id = D.hid[i];
  const int w = D.hw[i];
  int r = 0, ro = 0;
  bool first_max = w == nmax;
  for (int j = 0; j < m; j++) {
    const long long idj = D.hid[j];
    const int wj = D.hw[j];
    r += idj < id;
    // sort(vPairs) ascending, then push_front (src/KeyFrame.cc:459-467): weight descending, id descending
    if (wj >= th) ro += (wj > w) || (wj == w && idj > id);
    if (wj == nmax && idj < id) first_max = false;
  }
  D.ckf[r] = id;
  D.cw[r] = w;
  if (n_ord > 0) {
    if (w >= th) {
      D.okf[ro] = id;
      D.ow[ro] = w;
    }
  } else if (first_max) {  // :434-438: the first strictly greater count of an ascending walk
    D.okf[0] = id;
    D.ow[0] = w;
  }
}

// ---- UpdateLocalPoints: one block per listed keyframe
__global__ __launch_bounds__(256) void k_covis_lp_min(CvDev D, const int32_t* __restrict__ slots) {
  const CvMeta M = D.meta[slots[blockIdx.x]];
  for (int i = threadIdx.x; i < M.len; i += 256) {
    const int p = D.pid[M.off + i];
    if (p < 0 || D.bad[p]) continue;
    atomicMin(&D.minkey[p], ((unsigned long long)blockIdx.x << 32) | (unsigned)i);
  }
}

__global__ __launch_bounds__(256) void k_covis_lp_count(CvDev D, const int32_t* __restrict__ slots, int32_t* kcount) {
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const CvMeta M = D.meta[slots[blockIdx.x]];
  int n = 0;
  for (int i = threadIdx.x; i < M.len; i += 256) {
    const int p = D.pid[M.off + i];
    if (p < 0 || D.bad[p]) continue;
    n += D.minkey[p] == (((unsigned long long)blockIdx.x << 32) | (unsigned)i);
  }
  n = wave_sum(n);
  if ((threadIdx.x & 63) == 0) atomicAdd(&s_n, n);
  __syncthreads();
  if (threadIdx.x == 0) kcount[blockIdx.x] = s_n;
}

__global__ __launch_bounds__(256) void k_covis_lp_emit(CvDev D, const int32_t* __restrict__ slots,
                                                       const int32_t* __restrict__ kcount, int32_t* out) {
  __shared__ int s_base, s_wt[4];
  const int k = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  int b = 0;
  for (int j = threadIdx.x; j < k; j += 256) b += kcount[j];
  b = wave_sum(b);
  if (lane == 0 && b) atomicAdd(&s_base, b);
  __syncthreads();
  int run = s_base;  // winners of the keyframes listed before this one
  const CvMeta M = D.meta[slots[k]];
  for (int base = 0; base < M.len; base += 256) {  // (block-uniform trip count)
    const int i = base + threadIdx.x;
    int p = -1;
    bool win = false;
    if (i < M.len) {
      p = D.pid[M.off + i];
      // a later occurrence reads its point's key, the winner's or the wiped one: never its own
      win = p >= 0 && !D.bad[p] && D.minkey[p] == (((unsigned long long)k << 32) | (unsigned)i);
    }
    const unsigned long long m = __ballot(win);
    if (lane == 0) s_wt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 4; w++) {
      before += w < wave ? s_wt[w] : 0;
      all += s_wt[w];
    }
    if (win) {
      out[run + before + __popcll(m & ((1ull << lane) - 1ull))] = p;
      D.minkey[p] = ~0ull;  // wiped for the next query by the one entry that owns it
    }
    run += all;
    __syncthreads();
  }
  if (k == (int)gridDim.x - 1 && threadIdx.x == 0) D.ctl->n_win = run;
}

// ---- KeyFrameCulling
// mode 0: the candidates' non-bad points -> bitmap; 1: every per-point scratch word back to its rest value
__global__ __launch_bounds__(256) void k_covis_cull_mark(CvDev D, const int32_t* __restrict__ slots, int mode) {
  const CvMeta M = D.meta[slots[blockIdx.x]];
  if (mode == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    D.ctl->total = 0;
    D.ctl->n_bad = 0;
  }
  for (int i = threadIdx.x; i < M.len; i += 256) {
    const int p = D.pid[M.off + i];
    if (p < 0) continue;
    if (mode == 0) {
      if (!D.bad[p]) atomicOr(&D.bitmap[p >> 5], 1u << (p & 31));
    } else {
      D.bitmap[p >> 5] = 0u;
      D.pcnt[p] = 0;
      D.pfill[p] = 0;
      D.poff[p] = -1;
    }
  }
}

// mode 0: count every marked point's observers; 1: write them (slot << 8 | stereo << 7 | octave) into its list
__global__ __launch_bounds__(256) void k_covis_cull_lists(CvDev D, int mode) {
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv >= D.n_live) return;
  const int slot = D.live[wv];
  const CvMeta M = D.meta[slot];
  for (int i = lane; i < M.len; i += 64) {
    const int p = D.pid[M.off + i];
    if (p < 0 || !((D.bitmap[p >> 5] >> (p & 31)) & 1u)) continue;
    if (mode == 0) {
      atomicAdd(&D.pcnt[p], 1);
    } else {
      const uint8_t a = D.aux[M.off + i];
      const int pos = D.poff[p] + atomicAdd(&D.pfill[p], 1);
      D.list[pos] = ((uint32_t)slot << 8) | ((a & kAuxStereo) ? 0x80u : 0u) | (a & kAuxOct);
    }
  }
}

// every marked point's list gets its place: the first candidate entry to claim the point hands it out
__global__ __launch_bounds__(256) void k_covis_cull_off(CvDev D, const int32_t* __restrict__ slots) {
  const CvMeta M = D.meta[slots[blockIdx.x]];
  for (int i = threadIdx.x; i < M.len; i += 256) {
    const int p = D.pid[M.off + i];
    if (p < 0 || D.bad[p]) continue;
    if (atomicCAS(&D.poff[p], -1, -2) == -1) atomicExch(&D.poff[p], atomicAdd(&D.ctl->total, D.pcnt[p]));
  }
}

// src/LocalMapping.cc:796-870 as written: the candidates one after the other, because a culled keyframe's
// observations leave (src/KeyFrame.cc:585-587), its points' nObs drop and a point at nObs <= 2 turns bad
// (src/MapPoint.cc:121-138) for every candidate after it.  One workgroup; nothing waits for another block.
__global__ __launch_bounds__(kCullThreads) void k_covis_cull(CvDev D, const int32_t* __restrict__ slots,
                                                            const uint8_t* __restrict__ not_erase, int n_cand,
                                                            int monocular, uint8_t* verdict, int32_t* went_bad) {
  __shared__ int s_mp, s_red;
  const int tid = threadIdx.x, lane = tid & 63;
  for (int c = 0; c < n_cand; c++) {
    if (tid == 0) {
      s_mp = 0;
      s_red = 0;
    }
    __syncthreads();
    const int slot = slots[c];
    const CvMeta M = D.meta[slot];
    if (M.id == 0) {  // :799
      if (tid == 0) verdict[c] = 0;
      continue;  // (block-uniform)
    }
    int mp = 0, red = 0;
    for (int i = tid; i < M.len; i += kCullThreads) {
      const int p = D.pid[M.off + i];
      if (p < 0 || D.bad[p]) continue;  // :813-815
      const uint8_t a = D.aux[M.off + i];
      if (!monocular && !(a & kAuxClose)) continue;  // :818-822
      mp++;                                          // :824
      if (D.nobs[p] > 3) {                           // :826
        const int level = a & kAuxOct, o = D.poff[p], cn = D.pcnt[p];
        int n = 0;
        for (int e = 0; e < cn && n < 3; e++) {  // :834-854 (the count saturates at thObs)
          const uint32_t v = D.list[o + e];
          const int s2 = (int)(v >> 8);
          if (s2 == slot || !D.meta[s2].live) continue;  // :841, and the keyframes culled before this one
          if ((int)(v & kAuxOct) <= level + 1) n++;      // :847
        }
        red += n >= 3;  // :857-860
      }
    }
    mp = wave_sum(mp);
    red = wave_sum(red);
    if (lane == 0 && (mp | red)) {
      atomicAdd(&s_mp, mp);
      atomicAdd(&s_red, red);
    }
    __syncthreads();
    const bool cull = (double)s_red > 0.9 * (double)s_mp;  // :868, in double as written
    if (cull && !not_erase[c]) {
      if (tid == 0) D.meta[slot].live = 0;
      for (int i = tid; i < M.len; i += kCullThreads) {  // src/KeyFrame.cc:585-587
        const int p = D.pid[M.off + i];
        if (p < 0 || D.bad[p]) continue;
        const int w = (D.aux[M.off + i] & kAuxStereo) ? 2 : 1;
        if (atomicSub(&D.nobs[p], w) - w <= 2) {  // src/MapPoint.cc:132
          D.bad[p] = 1;                           // (a row holds a point once: one thread per point)
          went_bad[atomicAdd(&D.ctl->n_bad, 1)] = p;
        }
      }
    }
    if (tid == 0) verdict[c] = cull ? (not_erase[c] ? 2 : 1) : 0;
    __threadfence_block();
    __syncthreads();  // the next candidate reads live / nobs / bad as this one left them
  }
}

__global__ __launch_bounds__(256) void k_covis_compact(const CvMeta* __restrict__ meta, const int32_t* __restrict__ order,
                                                       const long long* __restrict__ new_off,
                                                       const int32_t* __restrict__ p0, const uint8_t* __restrict__ a0,
                                                       int32_t* __restrict__ p1, uint8_t* __restrict__ a1) {
  const CvMeta M = meta[order[blockIdx.x]];
  const long long o = new_off[blockIdx.x];
  for (int i = threadIdx.x; i < M.len; i += 256) {
    p1[o + i] = p0[M.off + i];
    a1[o + i] = a0[M.off + i];
  }
}

// the probes: a row with its bad points shown as -1; nObs and bad of listed points
__global__ __launch_bounds__(256) void k_covis_read_row(CvDev D, long long off, int len, int32_t* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  const int p = D.pid[off + i];
  out[i] = (p >= 0 && D.bad[p]) ? -1 : p;
  out[len + i] = D.aux[off + i];
}
__global__ __launch_bounds__(256) void k_covis_read_points(CvDev D, const int32_t* __restrict__ ids, int n, int32_t* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = D.nobs[ids[i]];
  out[n + i] = D.bad[ids[i]];
}
__global__ __launch_bounds__(256) void k_covis_set_bad(uint8_t* bad, const int32_t* __restrict__ ids, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) bad[ids[i]] = 1;
}

}  // namespace orbx

// ------------------------------------------------------------------ host / C ABI
using orbx::CvMeta;

struct orbx_covis {
  int device = 0;
  orbx::Stream st;  // (declared first: destroyed after everything below)
  // host mirrors (by slot; a slot is kept for every keyframe id seen since the last clear)
  std::unordered_map<long long, int> slot_of;
  std::vector<CvMeta> meta;
  std::vector<int32_t> live, live_pos;
  long long pool_used = 0, pool_cap = 0, pool_dead = 0;
  bool meta_dirty = false, live_dirty = false;
  int n_points = 0;  // largest point id seen + 1
  // device: the pool (repool replaces both)
  orbx::DevBuf<int32_t> d_pid;
  orbx::DevBuf<uint8_t> d_aux;
  orbx::DevBuf<uint32_t> d_list;  // cull's observer lists: never more entries than the pool
  int slot_cap = 0;
  orbx::DevBuf<CvMeta> d_meta;
  // the per-live query scratch (flush grows it)
  int live_cap = 0;
  orbx::DevBuf<int32_t> d_live, d_cnt, d_hw, d_cw, d_ow;
  orbx::DevBuf<long long> d_hid, d_ckf, d_okf;
  // the per-point tables (grow_points grows them together)
  int pcap = 0;
  orbx::DevBuf<int32_t> d_nobs, d_pcnt, d_pfill, d_poff;
  orbx::DevBuf<uint8_t> d_bad;
  orbx::DevBuf<uint32_t> d_bitmap;
  orbx::DevBuf<unsigned long long> d_minkey;
  orbx::DevBuf<orbx::CvCtl> d_ctl;
  orbx::CvCtl h_ctl{};
  // per-call staging, grown to what a call needs
  orbx::DevBuf<int32_t> d_q, d_slots, d_kcount, d_out;
  orbx::DevBuf<uint8_t> d_qb, d_ne, d_verdict;
};

namespace {

#define CV_CHECK(x)                             \
  do {                                          \
    if ((x) != hipSuccess) return ORBX_ERR_HIP; \
  } while (0)

// growth, as kfdb.hip's: tables double from 1,024 slots, the pool holds twice what is asked for and at least
// 65,536 entries, the per-point tables twice the largest id and at least 65,536 points
constexpr int table_slots(int n) { return 2 * n > 1024 ? 2 * n : 1024; }
constexpr long long pool_entries(long long n) { return 2 * n > (1 << 16) ? 2 * n : 1 << 16; }
constexpr int point_slots(int n) { return 2 * n > (1 << 16) ? 2 * n : 1 << 16; }
constexpr int kMaxSlots = 1 << 24;  // an observer-list entry keeps the slot in 24 bits

// a fresh array of new_n entries in place of *p, every byte `fill`, the first old_n entries kept when asked
template <class T>
hipError_t grow(orbx::DevBuf<T>* p, size_t old_n, size_t new_n, bool keep, int fill, hipStream_t st) {
  orbx::DevBuf<T> q;
  hipError_t e = q.ensure(new_n);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(q.p, fill, q.n * sizeof(T), st);
  if (e == hipSuccess && keep && p->p && old_n)
    e = hipMemcpyAsync(q.p, p->p, old_n * sizeof(T), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  p->swap(q);
  return hipSuccess;
}

orbx_status grow_points(orbx_covis* h, int32_t max_id) {
  if (max_id < 0) return ORBX_OK;
  h->n_points = std::max(h->n_points, (int)max_id + 1);
  if (max_id < h->pcap) return ORBX_OK;
  const int oc = h->pcap, nc = point_slots((int)max_id + 1);
  CV_CHECK(grow(&h->d_nobs, oc, nc, true, 0, h->st));
  CV_CHECK(grow(&h->d_bad, oc, nc, true, 0, h->st));
  CV_CHECK(grow(&h->d_pcnt, 0, nc, false, 0, h->st));
  CV_CHECK(grow(&h->d_pfill, 0, nc, false, 0, h->st));
  CV_CHECK(grow(&h->d_poff, 0, nc, false, 0xff, h->st));    // -1
  CV_CHECK(grow(&h->d_minkey, 0, nc, false, 0xff, h->st));  // ~0
  CV_CHECK(grow(&h->d_bitmap, 0, (size_t)nc / 32 + 1, false, 0, h->st));
  h->pcap = nc;
  return ORBX_OK;
}

orbx_status slot_for(orbx_covis* h, long long id, int* out) {
  auto it = h->slot_of.find(id);
  if (it != h->slot_of.end()) {
    *out = it->second;
    return ORBX_OK;
  }
  const int s = (int)h->meta.size();
  if (s >= kMaxSlots) return ORBX_ERR_CAPACITY;
  if (s >= h->slot_cap) {
    const int nc = table_slots(h->slot_cap);
    CV_CHECK(grow(&h->d_meta, 0, nc, false, 0, h->st));
    h->slot_cap = nc;
  }
  CvMeta m{};
  m.id = id;
  h->meta.push_back(m);
  h->live_pos.push_back(-1);
  h->slot_of.emplace(id, s);
  h->meta_dirty = true;
  *out = s;
  return ORBX_OK;
}

int live_slot(const orbx_covis* h, long long id) {
  auto it = h->slot_of.find(id);
  return (it == h->slot_of.end() || !h->meta[it->second].live) ? -1 : it->second;
}

// uploads what changed in the mirrors and sizes the per-live scratch
orbx_status flush(orbx_covis* h) {
  if (h->meta_dirty && !h->meta.empty())
    CV_CHECK(hipMemcpyAsync(h->d_meta.p, h->meta.data(), sizeof(CvMeta) * h->meta.size(), hipMemcpyHostToDevice, h->st));
  h->meta_dirty = false;
  const int nl = (int)h->live.size();
  if (nl > h->live_cap) {
    const int nc = table_slots(nl);
    CV_CHECK(h->d_live.ensure(nc));
    CV_CHECK(h->d_cnt.ensure(nc));
    CV_CHECK(h->d_hw.ensure(nc));
    CV_CHECK(h->d_cw.ensure(nc));
    CV_CHECK(h->d_ow.ensure(nc));
    CV_CHECK(h->d_hid.ensure(nc));
    CV_CHECK(h->d_ckf.ensure(nc));
    CV_CHECK(h->d_okf.ensure(nc));
    h->live_cap = nc;
    h->live_dirty = true;
  }
  if (h->live_dirty && nl > 0)
    CV_CHECK(hipMemcpyAsync(h->d_live.p, h->live.data(), 4 * (size_t)nl, hipMemcpyHostToDevice, h->st));
  h->live_dirty = false;
  // the mirrors may change right after this returns
  CV_CHECK(hipStreamSynchronize(h->st));
  return ORBX_OK;
}

orbx::CvDev dev_view(const orbx_covis* h) {
  orbx::CvDev D{};
  D.pid = h->d_pid.p;
  D.aux = h->d_aux.p;
  D.meta = h->d_meta.p;
  D.live = h->d_live.p;
  D.n_live = (int)h->live.size();
  D.pcap = h->pcap;
  D.nobs = h->d_nobs.p;
  D.bad = h->d_bad.p;
  D.bitmap = h->d_bitmap.p;
  D.minkey = h->d_minkey.p;
  D.pcnt = h->d_pcnt.p;
  D.pfill = h->d_pfill.p;
  D.poff = h->d_poff.p;
  D.list = h->d_list.p;
  D.cnt = h->d_cnt.p;
  D.hid = h->d_hid.p;
  D.hw = h->d_hw.p;
  D.ckf = h->d_ckf.p;
  D.cw = h->d_cw.p;
  D.okf = h->d_okf.p;
  D.ow = h->d_ow.p;
  D.ctl = h->d_ctl.p;
  return D;
}

int blocks(long long n, int per) { return (int)std::max<long long>(1, (n + per - 1) / per); }

// moves the live rows into a fresh pool with room for `extra` more entries
orbx_status repool(orbx_covis* h, long long extra) {
  const int nl = (int)h->live.size();
  std::vector<int32_t> order(h->live);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return h->meta[a].off < h->meta[b].off; });
  std::vector<long long> new_off(std::max(nl, 1));
  long long used = 0;
  for (int i = 0; i < nl; i++) {
    new_off[i] = used;
    used += h->meta[order[i]].len;
  }
  const long long cap = pool_entries(used + extra);
  orbx::DevBuf<int32_t> p1, d_order;
  orbx::DevBuf<uint8_t> a1;
  orbx::DevBuf<long long> d_off;
  hipError_t e = p1.ensure((size_t)cap);
  if (e == hipSuccess) e = a1.ensure((size_t)cap);
  if (e == hipSuccess && nl > 0 && used > 0) {
    if (flush(h) != ORBX_OK) e = hipErrorUnknown;  // the device still holds the old offsets
    if (e == hipSuccess) e = d_off.ensure((size_t)nl);
    if (e == hipSuccess) e = d_order.ensure((size_t)nl);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off.p, new_off.data(), 8 * (size_t)nl, hipMemcpyHostToDevice, h->st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_order.p, order.data(), 4 * (size_t)nl, hipMemcpyHostToDevice, h->st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(orbx::k_covis_compact, dim3(nl), dim3(256), 0, h->st, h->d_meta.p, d_order.p, d_off.p,
                         h->d_pid.p, h->d_aux.p, p1.p, a1.p);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->st);
  }
  if (e != hipSuccess) return ORBX_ERR_HIP;
  h->d_pid.swap(p1);
  h->d_aux.swap(a1);
  h->pool_cap = cap;
  h->pool_used = used;
  h->pool_dead = 0;
  for (int i = 0; i < nl; i++) h->meta[order[i]].off = new_off[i];
  h->meta_dirty = true;
  return ORBX_OK;
}

// takes a live row out: its nObs contributions leave, its pool entries are dead
orbx_status retire_row(orbx_covis* h, int slot, bool take_out) {
  CvMeta& m = h->meta[slot];
  if (take_out && m.len > 0) {
    hipLaunchKernelGGL(orbx::k_covis_row_apply, dim3(blocks(m.len, 256)), dim3(256), 0, h->st, h->d_pid.p, h->d_aux.p,
                       m.off, m.len, h->d_nobs.p, h->d_bad.p, -1);
    CV_CHECK(hipGetLastError());
  }
  m.live = 0;
  h->pool_dead += m.len;
  m.len = 0;
  const int pos = h->live_pos[slot], last = h->live.back();
  h->live[pos] = last;
  h->live_pos[last] = pos;
  h->live.pop_back();
  h->live_pos[slot] = -1;
  h->meta_dirty = h->live_dirty = true;
  if (h->live.empty()) h->pool_used = h->pool_dead = 0;  // nothing left to move
  return ORBX_OK;
}

// mark, vote, commit, rank and wipe for one source; leaves the counts in h->h_ctl
orbx_status run_vote(orbx_covis* h, const orbx::CvSrc& S, int self, int th) {
  orbx_status fs = flush(h);
  if (fs != ORBX_OK) return fs;
  const orbx::CvDev D = dev_view(h);
  const int nl = D.n_live;
  hipLaunchKernelGGL(orbx::k_covis_mark, dim3(blocks(S.n, 256)), dim3(256), 0, h->st, D, S, 0);
  if (nl > 0) {
    hipLaunchKernelGGL(orbx::k_covis_vote, dim3(blocks(nl, 4)), dim3(256), 0, h->st, D, self);
    hipLaunchKernelGGL(orbx::k_covis_commit, dim3(blocks(nl, 256)), dim3(256), 0, h->st, D, th);
    hipLaunchKernelGGL(orbx::k_covis_rank, dim3(blocks(nl, 256)), dim3(256), 0, h->st, D, th);
  }
  hipLaunchKernelGGL(orbx::k_covis_mark, dim3(blocks(S.n, 256)), dim3(256), 0, h->st, D, S, 1);
  CV_CHECK(hipGetLastError());
  CV_CHECK(hipMemcpyAsync(&h->h_ctl, h->d_ctl.p, sizeof(orbx::CvCtl), hipMemcpyDeviceToHost, h->st));
  CV_CHECK(hipStreamSynchronize(h->st));
  return ORBX_OK;
}

// the counter (ids ascending) and the ordered list of the vote just run
orbx_status copy_vote(orbx_covis* h, int64_t* ckf, int32_t* cw, int cap, int* n_counter, int64_t* okf, int32_t* ow,
                      int cap_o, int* n_ordered) {
  const int m = h->h_ctl.n_hit, no = m == 0 ? 0 : (h->h_ctl.n_ord > 0 ? h->h_ctl.n_ord : 1);
  *n_counter = m;
  *n_ordered = no;
  if (m > cap || no > cap_o) return ORBX_ERR_CAPACITY;
  if (m > 0) {
    CV_CHECK(hipMemcpy(ckf, h->d_ckf.p, 8 * (size_t)m, hipMemcpyDeviceToHost));
    CV_CHECK(hipMemcpy(cw, h->d_cw.p, 4 * (size_t)m, hipMemcpyDeviceToHost));
    CV_CHECK(hipMemcpy(okf, h->d_okf.p, 8 * (size_t)no, hipMemcpyDeviceToHost));
    CV_CHECK(hipMemcpy(ow, h->d_ow.p, 4 * (size_t)no, hipMemcpyDeviceToHost));
  }
  return ORBX_OK;
}

// the live slots of a list of keyframe ids (already checked for repeats), on the device in d_slots
orbx_status upload_slots(orbx_covis* h, const int64_t* ids, int n, std::vector<int32_t>* slots) {
  slots->resize((size_t)std::max(n, 1));
  for (int i = 0; i < n; i++) {
    const int s = live_slot(h, (long long)ids[i]);
    if (s < 0) return ORBX_ERR_ARG;
    (*slots)[i] = s;
  }
  return ORBX_OK;
}

}  // namespace

extern "C" {

orbx_status orbx_covis_check_row(const int32_t* point_ids, const int32_t* octaves, const uint8_t* flags, int n) {
  return orbx::covis_row_ok(point_ids, octaves, flags, n) ? ORBX_OK : ORBX_ERR_ARG;
}

orbx_status orbx_covis_create(int device, orbx_covis** out) {
  if (!out) return ORBX_ERR_ARG;
  *out = nullptr;
  if (device < 0) return ORBX_ERR_ARG;
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return ORBX_ERR_NODEV;
  if (device >= nd) return ORBX_ERR_ARG;
  CV_CHECK(hipSetDevice(device));
  orbx_covis* h = new (std::nothrow) orbx_covis();
  if (!h) return ORBX_ERR_HIP;
  h->device = device;
  hipError_t e = h->st.ensure();
  if (e == hipSuccess) e = grow(&h->d_ctl, 0, 1, false, 0, h->st);
  if (e == hipSuccess && grow_points(h, 0) != ORBX_OK) e = hipErrorUnknown;
  h->n_points = 0;
  if (e != hipSuccess) {
    orbx_covis_destroy(h);
    return ORBX_ERR_HIP;
  }
  *out = h;
  return ORBX_OK;
}

orbx_status orbx_covis_destroy(orbx_covis* h) {
  if (!h) return ORBX_ERR_ARG;
  (void)hipSetDevice(h->device);
  if (h->st) (void)hipStreamSynchronize(h->st);
  delete h;
  return ORBX_OK;
}

orbx_status orbx_covis_clear(orbx_covis* h) {
  if (!h) return ORBX_ERR_ARG;
  CV_CHECK(hipSetDevice(h->device));
  CV_CHECK(hipMemsetAsync(h->d_nobs.p, 0, 4 * (size_t)h->pcap, h->st));
  CV_CHECK(hipMemsetAsync(h->d_bad.p, 0, (size_t)h->pcap, h->st));
  CV_CHECK(hipStreamSynchronize(h->st));
  h->slot_of.clear();
  h->meta.clear();
  h->live.clear();
  h->live_pos.clear();
  h->pool_used = h->pool_dead = 0;
  h->n_points = 0;
  h->meta_dirty = h->live_dirty = false;
  return ORBX_OK;
}

orbx_status orbx_covis_set_keyframe(orbx_covis* h, int64_t kf_id, int n, const int32_t* point_ids,
                                    const int32_t* octaves, const uint8_t* flags) {
  if (!h || kf_id < 0) return ORBX_ERR_ARG;
  if (!orbx::covis_row_ok(point_ids, octaves, flags, n)) return ORBX_ERR_ARG;
  CV_CHECK(hipSetDevice(h->device));
  orbx_status s = grow_points(h, orbx::covis_max_point(point_ids, n));
  if (s != ORBX_OK) return s;
  int slot = -1;
  s = slot_for(h, (long long)kf_id, &slot);
  if (s != ORBX_OK) return s;
  if (h->meta[slot].live) {  // a replacement: the old row's contributions leave first
    s = retire_row(h, slot, true);
    if (s != ORBX_OK) return s;
  }
  if (h->pool_used + n > h->pool_cap) {
    s = repool(h, n);  // grows (and drops the dead entries on the way)
    if (s != ORBX_OK) return s;
  }
  CvMeta& m = h->meta[slot];
  m.off = h->pool_used;
  m.len = n;
  m.live = 1;
  if (n > 0) {
    std::vector<uint8_t> aux((size_t)n);
    for (int i = 0; i < n; i++)
      aux[i] = (uint8_t)(octaves[i] | ((flags[i] & orbx::kCovisStereo) ? orbx::kAuxStereo : 0) |
                         ((flags[i] & orbx::kCovisClose) ? orbx::kAuxClose : 0));
    hipError_t e = hipMemcpyAsync(h->d_pid.p + m.off, point_ids, 4 * (size_t)n, hipMemcpyHostToDevice, h->st);
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_aux.p + m.off, aux.data(), (size_t)n, hipMemcpyHostToDevice, h->st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(orbx::k_covis_row_apply, dim3(blocks(n, 256)), dim3(256), 0, h->st, h->d_pid.p, h->d_aux.p,
                         m.off, n, h->d_nobs.p, h->d_bad.p, 1);
      e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(h->st);  // the caller's arrays and aux are free again
    if (e != hipSuccess || e2 != hipSuccess) {
      m.live = 0;
      m.len = 0;
      return ORBX_ERR_HIP;
    }
  }
  h->pool_used += n;
  h->live_pos[slot] = (int)h->live.size();
  h->live.push_back(slot);
  h->meta_dirty = h->live_dirty = true;
  return ORBX_OK;
}

orbx_status orbx_covis_erase_keyframe(orbx_covis* h, int64_t kf_id) {
  if (!h) return ORBX_ERR_ARG;
  const int slot = live_slot(h, (long long)kf_id);
  if (slot < 0) return ORBX_ERR_ARG;
  CV_CHECK(hipSetDevice(h->device));
  orbx_status s = retire_row(h, slot, true);
  if (s != ORBX_OK) return s;
  CV_CHECK(hipStreamSynchronize(h->st));
  if (!h->live.empty() && 2 * h->pool_dead > h->pool_used) return repool(h, 0);  // more dead than live: compact
  return ORBX_OK;
}

orbx_status orbx_covis_set_points_bad(orbx_covis* h, const int32_t* ids, int n) {
  if (!h || !orbx::covis_point_list_ok(ids, n, false)) return ORBX_ERR_ARG;
  if (n == 0) return ORBX_OK;
  CV_CHECK(hipSetDevice(h->device));
  orbx_status s = grow_points(h, orbx::covis_max_point(ids, n));
  if (s != ORBX_OK) return s;
  CV_CHECK(h->d_q.ensure((size_t)n));
  hipError_t e = hipMemcpyAsync(h->d_q.p, ids, 4 * (size_t)n, hipMemcpyHostToDevice, h->st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(orbx::k_covis_set_bad, dim3(blocks(n, 256)), dim3(256), 0, h->st, h->d_bad.p, h->d_q.p, n);
    e = hipGetLastError();
  }
  const hipError_t e2 = hipStreamSynchronize(h->st);
  return (e == hipSuccess && e2 == hipSuccess) ? ORBX_OK : ORBX_ERR_HIP;
}

orbx_status orbx_covis_size(const orbx_covis* h, int* live, long long* pool_entries, int* n_points) {
  if (!h) return ORBX_ERR_ARG;
  if (live) *live = (int)h->live.size();
  if (pool_entries) *pool_entries = h->pool_used;
  if (n_points) *n_points = h->n_points;
  return ORBX_OK;
}

orbx_status orbx_covis_read_keyframe(orbx_covis* h, int64_t kf_id, int32_t* point_ids, int32_t* octaves,
                                     uint8_t* flags, int cap, int* n) {
  if (!h || !n || cap < 0 || (cap > 0 && (!point_ids || !octaves || !flags))) return ORBX_ERR_ARG;
  const int slot = live_slot(h, (long long)kf_id);
  if (slot < 0) return ORBX_ERR_ARG;
  const CvMeta m = h->meta[slot];
  *n = m.len;
  if (m.len > cap) return ORBX_ERR_CAPACITY;
  if (m.len == 0) return ORBX_OK;
  CV_CHECK(hipSetDevice(h->device));
  CV_CHECK(h->d_out.ensure(2 * (size_t)m.len));
  std::vector<int32_t> out(2 * (size_t)m.len);
  hipLaunchKernelGGL(orbx::k_covis_read_row, dim3(blocks(m.len, 256)), dim3(256), 0, h->st, dev_view(h), m.off, m.len,
                     h->d_out.p);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out.data(), h->d_out.p, 4 * out.size(), hipMemcpyDeviceToHost, h->st);
  const hipError_t e2 = hipStreamSynchronize(h->st);
  if (e != hipSuccess || e2 != hipSuccess) return ORBX_ERR_HIP;
  for (int i = 0; i < m.len; i++) {
    const int a = out[(size_t)m.len + i];
    point_ids[i] = out[i];
    octaves[i] = a & orbx::kAuxOct;
    flags[i] = (uint8_t)(((a & orbx::kAuxStereo) ? orbx::kCovisStereo : 0) | ((a & orbx::kAuxClose) ? orbx::kCovisClose : 0));
  }
  return ORBX_OK;
}

orbx_status orbx_covis_read_points(orbx_covis* h, const int32_t* ids, int n, int32_t* n_obs, uint8_t* bad) {
  if (!h || !orbx::covis_point_list_ok(ids, n, false) || (n > 0 && (!n_obs || !bad))) return ORBX_ERR_ARG;
  for (int i = 0; i < n; i++)
    if (ids[i] >= h->n_points) return ORBX_ERR_ARG;  // never seen
  if (n == 0) return ORBX_OK;
  CV_CHECK(hipSetDevice(h->device));
  CV_CHECK(h->d_q.ensure((size_t)n));
  CV_CHECK(h->d_out.ensure(2 * (size_t)n));
  std::vector<int32_t> out(2 * (size_t)n);
  hipError_t e = hipMemcpyAsync(h->d_q.p, ids, 4 * (size_t)n, hipMemcpyHostToDevice, h->st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(orbx::k_covis_read_points, dim3(blocks(n, 256)), dim3(256), 0, h->st, dev_view(h), h->d_q.p, n,
                       h->d_out.p);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out.data(), h->d_out.p, 4 * out.size(), hipMemcpyDeviceToHost, h->st);
  const hipError_t e2 = hipStreamSynchronize(h->st);
  if (e != hipSuccess || e2 != hipSuccess) return ORBX_ERR_HIP;
  for (int i = 0; i < n; i++) {
    n_obs[i] = out[i];
    bad[i] = (uint8_t)out[(size_t)n + i];
  }
  return ORBX_OK;
}

orbx_status orbx_covis_update_connections(orbx_covis* h, int64_t kf_id, int th, int64_t* counter_kfs,
                                          int32_t* counter_w, int cap, int* n_counter, int64_t* ordered_kfs,
                                          int32_t* ordered_w, int cap_ordered, int* n_ordered) {
  if (!h || !n_counter || !n_ordered || cap < 0 || cap_ordered < 0 || (cap > 0 && (!counter_kfs || !counter_w)) ||
      (cap_ordered > 0 && (!ordered_kfs || !ordered_w)))
    return ORBX_ERR_ARG;
  const int slot = live_slot(h, (long long)kf_id);
  if (slot < 0) return ORBX_ERR_ARG;
  CV_CHECK(hipSetDevice(h->device));
  orbx::CvSrc S{};
  S.ids = h->d_pid.p;
  S.off = h->meta[slot].off;
  S.n = h->meta[slot].len;
  orbx_status s = run_vote(h, S, slot, th);
  if (s != ORBX_OK) return s;
  return copy_vote(h, counter_kfs, counter_w, cap, n_counter, ordered_kfs, ordered_w, cap_ordered, n_ordered);
}

orbx_status orbx_covis_vote(orbx_covis* h, const int32_t* point_ids, int n, uint8_t* was_bad, int64_t* kfs,
                            int32_t* counts, int cap, int* n_kfs, int64_t* kf_max, int32_t* n_max) {
  if (!h || !n_kfs || !kf_max || !n_max || cap < 0 || (cap > 0 && (!kfs || !counts)) || (n > 0 && !was_bad))
    return ORBX_ERR_ARG;
  if (!orbx::covis_point_list_ok(point_ids, n, true)) return ORBX_ERR_ARG;
  CV_CHECK(hipSetDevice(h->device));
  CV_CHECK(h->d_q.ensure((size_t)n));
  CV_CHECK(h->d_qb.ensure((size_t)n));
  if (n > 0) CV_CHECK(hipMemcpyAsync(h->d_q.p, point_ids, 4 * (size_t)n, hipMemcpyHostToDevice, h->st));
  orbx::CvSrc S{};
  S.ids = h->d_q.p;
  S.n = n;
  S.was_bad = h->d_qb.p;
  orbx_status s = run_vote(h, S, -1, INT_MAX);  // nothing reaches th: the ordered list is (max, pKFmax)
  if (s != ORBX_OK) return s;
  if (n > 0) CV_CHECK(hipMemcpy(was_bad, h->d_qb.p, (size_t)n, hipMemcpyDeviceToHost));
  int no = 0;
  *kf_max = -1;
  *n_max = 0;
  return copy_vote(h, kfs, counts, cap, n_kfs, kf_max, n_max, 1, &no);
}

orbx_status orbx_covis_local_points(orbx_covis* h, const int64_t* kf_ids, int n_kfs, int32_t* point_ids, int cap,
                                    int* n_points) {
  if (!h || !n_points || cap < 0 || (cap > 0 && !point_ids)) return ORBX_ERR_ARG;
  if (!orbx::covis_kf_list_ok(kf_ids, n_kfs)) return ORBX_ERR_ARG;
  std::vector<int32_t> slots;
  orbx_status s = upload_slots(h, kf_ids, n_kfs, &slots);
  if (s != ORBX_OK) return s;
  *n_points = 0;
  if (n_kfs == 0) return ORBX_OK;
  long long total = 0;
  for (int i = 0; i < n_kfs; i++) total += h->meta[slots[i]].len;
  CV_CHECK(hipSetDevice(h->device));
  s = flush(h);
  if (s != ORBX_OK) return s;
  CV_CHECK(h->d_slots.ensure((size_t)n_kfs));
  CV_CHECK(h->d_kcount.ensure((size_t)n_kfs));
  CV_CHECK(h->d_out.ensure((size_t)total));
  const orbx::CvDev D = dev_view(h);
  hipError_t e = hipMemcpyAsync(h->d_slots.p, slots.data(), 4 * (size_t)n_kfs, hipMemcpyHostToDevice, h->st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(orbx::k_covis_lp_min, dim3(n_kfs), dim3(256), 0, h->st, D, h->d_slots.p);
    hipLaunchKernelGGL(orbx::k_covis_lp_count, dim3(n_kfs), dim3(256), 0, h->st, D, h->d_slots.p, h->d_kcount.p);
    hipLaunchKernelGGL(orbx::k_covis_lp_emit, dim3(n_kfs), dim3(256), 0, h->st, D, h->d_slots.p, h->d_kcount.p,
                       h->d_out.p);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&h->h_ctl, h->d_ctl.p, sizeof(orbx::CvCtl), hipMemcpyDeviceToHost, h->st);
  const hipError_t e2 = hipStreamSynchronize(h->st);
  if (e != hipSuccess || e2 != hipSuccess) return ORBX_ERR_HIP;
  const int m = h->h_ctl.n_win;
  *n_points = m;
  if (m > cap) return ORBX_ERR_CAPACITY;
  if (m > 0) CV_CHECK(hipMemcpy(point_ids, h->d_out.p, 4 * (size_t)m, hipMemcpyDeviceToHost));
  return ORBX_OK;
}

orbx_status orbx_covis_cull(orbx_covis* h, const int64_t* cand_ids, int n_cand, const uint8_t* not_erase,
                            int monocular, uint8_t* verdict, int32_t* bad_ids, int cap, int* n_bad) {
  if (!h || !n_bad || cap < 0 || (cap > 0 && !bad_ids) || (n_cand > 0 && (!not_erase || !verdict)))
    return ORBX_ERR_ARG;
  if (!orbx::covis_kf_list_ok(cand_ids, n_cand)) return ORBX_ERR_ARG;
  std::vector<int32_t> slots;
  orbx_status s = upload_slots(h, cand_ids, n_cand, &slots);
  if (s != ORBX_OK) return s;
  *n_bad = 0;
  if (n_cand == 0) return ORBX_OK;
  long long total = 0;
  for (int i = 0; i < n_cand; i++) total += h->meta[slots[i]].len;
  CV_CHECK(hipSetDevice(h->device));
  s = flush(h);
  if (s != ORBX_OK) return s;
  CV_CHECK(h->d_slots.ensure((size_t)n_cand));
  CV_CHECK(h->d_ne.ensure((size_t)n_cand));
  CV_CHECK(h->d_verdict.ensure((size_t)n_cand));
  CV_CHECK(h->d_out.ensure((size_t)total));
  CV_CHECK(h->d_list.ensure((size_t)std::max<long long>(h->pool_cap, 1)));
  const orbx::CvDev D = dev_view(h);
  const int nl = D.n_live;
  std::vector<int32_t> went((size_t)std::max<long long>(total, 1));
  hipError_t e = hipMemcpyAsync(h->d_slots.p, slots.data(), 4 * (size_t)n_cand, hipMemcpyHostToDevice, h->st);
  if (e == hipSuccess) e = hipMemcpyAsync(h->d_ne.p, not_erase, (size_t)n_cand, hipMemcpyHostToDevice, h->st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(orbx::k_covis_cull_mark, dim3(n_cand), dim3(256), 0, h->st, D, h->d_slots.p, 0);
    hipLaunchKernelGGL(orbx::k_covis_cull_lists, dim3(blocks(nl, 4)), dim3(256), 0, h->st, D, 0);
    hipLaunchKernelGGL(orbx::k_covis_cull_off, dim3(n_cand), dim3(256), 0, h->st, D, h->d_slots.p);
    hipLaunchKernelGGL(orbx::k_covis_cull_lists, dim3(blocks(nl, 4)), dim3(256), 0, h->st, D, 1);
    hipLaunchKernelGGL(orbx::k_covis_cull, dim3(1), dim3(orbx::kCullThreads), 0, h->st, D, h->d_slots.p, h->d_ne.p,
                       n_cand, monocular ? 1 : 0, h->d_verdict.p, h->d_out.p);
    hipLaunchKernelGGL(orbx::k_covis_cull_mark, dim3(n_cand), dim3(256), 0, h->st, D, h->d_slots.p, 1);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(verdict, h->d_verdict.p, (size_t)n_cand, hipMemcpyDeviceToHost, h->st);
  if (e == hipSuccess) e = hipMemcpyAsync(&h->h_ctl, h->d_ctl.p, sizeof(orbx::CvCtl), hipMemcpyDeviceToHost, h->st);
  hipError_t e2 = hipStreamSynchronize(h->st);
  if (e != hipSuccess || e2 != hipSuccess) return ORBX_ERR_HIP;
  const int m = h->h_ctl.n_bad;
  if (m > 0) CV_CHECK(hipMemcpy(went.data(), h->d_out.p, 4 * (size_t)m, hipMemcpyDeviceToHost));
  // the mirrors follow the device: the culled rows are retired (their contributions left in the kernel)
  for (int c = 0; c < n_cand; c++)
    if (verdict[c] == 1) (void)retire_row(h, slots[c], false);
  if (!h->live.empty() && 2 * h->pool_dead > h->pool_used) {
    s = repool(h, 0);
    if (s != ORBX_OK) return s;
  }
  *n_bad = m;
  if (m > cap) return ORBX_ERR_CAPACITY;
  std::sort(went.begin(), went.begin() + m);  // ascending ids: the list's order of arrival never leaves
  if (m > 0) std::memcpy(bad_ids, went.data(), 4 * (size_t)m);
  return ORBX_OK;
}

}  // extern "C"

// kfdb.hip -- KeyFrameDatabase (src/KeyFrameDatabase.cc:33-341) as a device-resident object:
// DetectRelocalizationCandidates (:219-341), DetectLoopCandidates (:76-217) and
// ORBVocabulary::score (DBoW2 L1Scoring::score, restated from upstream: ScoringObject.cpp is not in
// the reference tree) with the reference's exact results, candidate order and per-keyframe state.
//
// The map is scanned, not indexed: the live keyframes' BowVectors lie in one CSR pool (words u32,
// values f64 apart) and a query tests every keyframe word against a bitmap of the query's words.
// The reference's lKFsSharingWords order (query words ascending, each word's list in add order) is
// the ascending order of the key (smallest common word, add sequence number), so no list exists.
//
//   k_kfdb_begin    query words -> bitmap (n_words bits), connected set -> byte marks, counters reset
//   k_kfdb_vote     one wave per live keyframe: common words (mn*Words), smallest common word, the
//                   L1 score summed over the common words in ascending word order by the wave's hit
//                   lanes one after the other (bit-exact double), state update of :100-112 / :237-243,
//                   integer atomicMax for maxCommonWords
//   k_kfdb_commit   minCommonWords = maxCommonWords*0.8f; m*Score of the keyframes above it; the
//                   bitmap and the connected marks are wiped for the next query
//   k_kfdb_acc      one thread per scored keyframe: its <= 10 neighbours in order, float accScore,
//                   pBestKF; atomicMax for bestAccScore
//   k_kfdb_mark     entries above 0.75f*bestAccScore: per pBestKF the smallest key pointing at it
//   k_kfdb_win      the entry that owns that smallest key is the first occurrence of its pBestKF
//   k_kfdb_rank     rank of every winner's key among the winners = its place in the output
//   k_kfdb_score    ORBVocabulary::score for a list of keyframes
//   k_kfdb_compact  moves the live keyframes' pool entries to a fresh pool
// Only k_kfdb_rank's order matters, and it ranks by key, so every atomic above is order-free.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

#include "../../include/orbx.h"
#include "orbx_mem.h"

namespace orbx {

constexpr int kKfdbMaxQuery = 8192;  // words of one BowVector (a frame carries <= 8192 features)
constexpr int kKfdbNeigh = 10;       // GetBestCovisibilityKeyFrames(10)
constexpr int kKfdbConnRing = 4;

struct KfMeta {
  long long off;  // first pool entry
  long long id;   // the caller's keyframe id (mnId)
  int32_t len;    // BowVector entries
  uint32_t seq;   // add sequence number (order within one word's inverted list)
  int32_t live;
  int32_t pad;
};

struct KfCtl {
  int max_common;
  unsigned best_acc;  // ordered-integer image of the float
  int n_win;
  int pad;
};

struct KfDev {
  const uint32_t* words;
  const double* vals;
  const KfMeta* meta;
  const int32_t* live;
  int n_live;
  const int32_t* neigh;  // slot x 10, -1 = none
  unsigned long long* rq;
  int32_t* rw;
  float* rs;
  unsigned long long* lq;
  int32_t* lw;
  float* ls;
  uint32_t* bitmap;
  unsigned n_words;
  uint8_t* conn;                // per slot: in the query's connected set
  unsigned long long* minkey;   // per slot: smallest key of a retained entry whose pBestKF it is
  // per live index
  unsigned long long* key;
  float* si;
  int32_t* flag;  // bit0: in lKFsSharingWords, bit1: in lScoreAndMatch
  float* acc;
  int32_t* best;
  unsigned long long* wkey;
  long long* wid;
  KfCtl* ctl;
};

struct KfQuery {
  const uint32_t* words;
  const double* vals;
  const int32_t* n;
  unsigned long long qid;
  int loop;
  float min_score;
  const int32_t* conn_list;  // slots
  int n_conn;
  long long* cand;
  int cap;
  int32_t* n_cand;
};

__device__ __forceinline__ unsigned f2ord(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ int qlen(const int32_t* n) { return min(max(*n, 0), kKfdbMaxQuery); }

__device__ __forceinline__ void bitmap_set(uint32_t* bm, unsigned n_words, const uint32_t* qw, int qn, int i) {
  if (i < qn) {
    const uint32_t w = qw[i];
    if (w < n_words) atomicOr(&bm[w >> 5], 1u << (w & 31));
  }
}
__device__ __forceinline__ void bitmap_wipe(uint32_t* bm, unsigned n_words, const uint32_t* qw, int qn, int i) {
  if (i < qn) {
    const uint32_t w = qw[i];
    if (w < n_words) bm[w >> 5] = 0u;
  }
}

// One wave, one keyframe: lanes stride over its words.  hits = common words, minw = the smallest of
// them, sum = L1Scoring::score's running sum, the terms added in ascending word order (chunk after
// chunk, within a chunk the hit lanes in lane order), every lane holding the same double.
__device__ __forceinline__ void wave_match(const uint32_t* __restrict__ words, const double* __restrict__ vals,
                                           const uint32_t* __restrict__ bitmap, unsigned n_words,
                                           const uint32_t* __restrict__ qw, const double* __restrict__ qv, int qn,
                                           long long off, int len, int lane, int* hits, uint32_t* minw,
                                           double* sum) {
  int h = 0;
  uint32_t mw = 0xffffffffu;
  double s = 0.0;
  for (int base = 0; base < len; base += 64) {
    const int i = base + lane;
    bool hit = false;
    uint32_t w = 0;
    if (i < len) {
      w = words[off + i];
      hit = w < n_words && ((bitmap[w >> 5] >> (w & 31)) & 1u);
    }
    const unsigned long long m = __ballot(hit);
    if (!m) continue;  // wave-uniform
    double t = 0.0;
    if (hit) {
      int lo = 0, hi = qn;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (qw[mid] < w)
          lo = mid + 1;
        else
          hi = mid;
      }
      if (lo >= qn) lo = qn - 1;  // cannot happen for an ascending query; keeps the read in bounds
      const double vi = qv[lo], wi = vals[off + i];
      t = (fabs(vi - wi) - fabs(vi)) - fabs(wi);
    }
    if (h == 0) mw = (uint32_t)__shfl((int)w, __ffsll((long long)m) - 1, 64);
    h += __popcll(m);
    unsigned long long r = m;
    while (r) {
      const int l = __ffsll((long long)r) - 1;
      s += __shfl(t, l, 64);
      r &= r - 1;
    }
  }
  *hits = h;
  *minw = mw;
  *sum = s;
}

__global__ __launch_bounds__(256) void k_kfdb_begin(KfDev D, KfQuery Q) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    D.ctl->max_common = 0;
    D.ctl->best_acc = f2ord(Q.loop ? Q.min_score : 0.f);
    D.ctl->n_win = 0;
  }
  bitmap_set(D.bitmap, D.n_words, Q.words, qlen(Q.n), i);
  if (i < Q.n_conn) D.conn[Q.conn_list[i]] = 1;
}

__global__ __launch_bounds__(256) void k_kfdb_vote(KfDev D, KfQuery Q) {
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv >= D.n_live) return;
  const int slot = D.live[wv];
  const KfMeta M = D.meta[slot];
  int hits;
  uint32_t mw;
  double s;
  wave_match(D.words, D.vals, D.bitmap, D.n_words, Q.words, Q.vals, qlen(Q.n), M.off, M.len, lane, &hits, &mw, &s);
  if (lane) return;
  D.minkey[slot] = ~0ull;
  int flag = 0;
  if (hits > 0) {
    if (!Q.loop) {  // :237-243
      if (D.rq[slot] != Q.qid) {
        D.rq[slot] = Q.qid;
        D.rw[slot] = hits;
        flag = 1;
      } else {
        D.rw[slot] += hits;
      }
    } else {  // :100-112
      if (D.lq[slot] != Q.qid) {
        if (D.conn[slot]) {
          D.lw[slot] = 1;  // reset at every encounter, never marked: one word, query id unchanged
        } else {
          D.lq[slot] = Q.qid;
          D.lw[slot] = hits;
          flag = 1;
        }
      } else {
        D.lw[slot] += hits;
      }
    }
    if (flag) atomicMax(&D.ctl->max_common, hits);
  }
  D.key[wv] = ((unsigned long long)mw << 32) | M.seq;
  D.si[wv] = (float)(-s / 2.0);
  D.flag[wv] = flag;
}

__global__ __launch_bounds__(256) void k_kfdb_commit(KfDev D, KfQuery Q) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bitmap_wipe(D.bitmap, D.n_words, Q.words, qlen(Q.n), i);
  if (i < Q.n_conn) D.conn[Q.conn_list[i]] = 0;
  if (i >= D.n_live || !D.flag[i]) return;
  const int slot = D.live[i];
  const int minc = (int)((float)D.ctl->max_common * 0.8f);
  const float si = D.si[i];
  if (!Q.loop) {
    if (D.rw[slot] > minc) {
      D.rs[slot] = si;
      D.flag[i] = 3;
    }
  } else if (D.lw[slot] > minc) {
    D.ls[slot] = si;
    if (si >= Q.min_score) D.flag[i] = 3;
  }
}

__global__ __launch_bounds__(256) void k_kfdb_acc(KfDev D, KfQuery Q) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.n_live || !(D.flag[i] & 2)) return;
  const int slot = D.live[i];
  const int minc = (int)((float)D.ctl->max_common * 0.8f);
  float best_score = D.si[i], acc = best_score;
  int best = slot;
  for (int j = 0; j < kKfdbNeigh; j++) {
    const int nb = D.neigh[(size_t)slot * kKfdbNeigh + j];
    if (nb < 0 || !D.meta[nb].live) continue;
    float sc;
    if (!Q.loop) {
      if (D.rq[nb] != Q.qid) continue;
      sc = D.rs[nb];
    } else {
      if (!(D.lq[nb] == Q.qid && D.lw[nb] > minc)) continue;
      sc = D.ls[nb];
    }
    acc += sc;
    if (sc > best_score) {
      best = nb;
      best_score = sc;
    }
  }
  D.acc[i] = acc;
  D.best[i] = best;
  atomicMax(&D.ctl->best_acc, f2ord(acc));
}

__global__ __launch_bounds__(256) void k_kfdb_mark(KfDev D) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.n_live || !(D.flag[i] & 2)) return;
  if (D.acc[i] > 0.75f * ord2f(D.ctl->best_acc)) atomicMin(&D.minkey[D.best[i]], D.key[i]);
}

__global__ __launch_bounds__(256) void k_kfdb_win(KfDev D) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.n_live || !(D.flag[i] & 2)) return;
  if (!(D.acc[i] > 0.75f * ord2f(D.ctl->best_acc))) return;
  const int best = D.best[i];
  if (D.minkey[best] != D.key[i]) return;  // a later occurrence of the same pBestKF (spAlreadyAddedKF)
  const int pos = atomicAdd(&D.ctl->n_win, 1);
  D.wkey[pos] = D.key[i];
  D.wid[pos] = D.meta[best].id;
}

__global__ __launch_bounds__(256) void k_kfdb_rank(KfDev D, KfQuery Q) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int m = D.ctl->n_win;
  if (i == 0) *Q.n_cand = m;
  if (i >= m) return;
  const unsigned long long k = D.wkey[i];
  int r = 0;
  for (int j = 0; j < m; j++) r += D.wkey[j] < k;
  if (r < Q.cap) Q.cand[r] = D.wid[i];
}

// mode 0: set the query's bits, 1: wipe them
__global__ __launch_bounds__(256) void k_kfdb_bitmap(uint32_t* bm, unsigned n_words, const uint32_t* qw,
                                                     const int32_t* qn, int mode) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (mode == 0)
    bitmap_set(bm, n_words, qw, qlen(qn), i);
  else
    bitmap_wipe(bm, n_words, qw, qlen(qn), i);
}

__global__ __launch_bounds__(256) void k_kfdb_score(KfDev D, const uint32_t* qw, const double* qv, const int32_t* qn,
                                                    const int32_t* slots, int n, double* out) {
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv >= n) return;
  const KfMeta M = D.meta[slots[wv]];
  int hits;
  uint32_t mw;
  double s;
  wave_match(D.words, D.vals, D.bitmap, D.n_words, qw, qv, qlen(qn), M.off, M.len, lane, &hits, &mw, &s);
  if (lane == 0) out[wv] = -s / 2.0;
}

__global__ __launch_bounds__(256) void k_kfdb_compact(const KfMeta* __restrict__ meta, const int32_t* __restrict__ live,
                                                      const long long* __restrict__ new_off,
                                                      const uint32_t* __restrict__ w0, const double* __restrict__ v0,
                                                      uint32_t* __restrict__ w1, double* __restrict__ v1) {
  const KfMeta M = meta[live[blockIdx.x]];
  const long long o = new_off[blockIdx.x];
  for (int i = threadIdx.x; i < M.len; i += 256) {
    w1[o + i] = w0[M.off + i];
    v1[o + i] = v0[M.off + i];
  }
}

}  // namespace orbx

// ------------------------------------------------------------------ host / C ABI
using orbx::KfMeta;

struct orbx_kfdb {
  int device = 0;
  orbx::Stream st;  // (declared first: destroyed after everything below)
  orbx::Event ev;   // end of the last queued query
  bool ev_set = false;
  unsigned n_words = 0;
  // host mirrors (by slot; a slot is kept for every id ever seen, so its state survives erase + add)
  std::unordered_map<long long, int> slot_of;
  std::vector<KfMeta> meta;
  std::vector<int32_t> neigh;
  std::vector<int32_t> live, live_pos;
  long long pool_used = 0, pool_cap = 0, pool_dead = 0;
  uint32_t next_seq = 0;
  int meta_lo = 0, meta_hi = 0, neigh_lo = 0, neigh_hi = 0;  // dirty slot ranges [lo, hi)
  bool live_dirty = false;
  // device: the pool (repool replaces both)
  orbx::DevBuf<uint32_t> d_words;
  orbx::DevBuf<double> d_vals;
  // the per-slot tables (slot_for grows them together)
  int slot_cap = 0;
  orbx::DevBuf<KfMeta> d_meta;
  orbx::DevBuf<int32_t> d_neigh;
  orbx::DevBuf<unsigned long long> d_rq, d_lq, d_minkey;
  orbx::DevBuf<int32_t> d_rw, d_lw;
  orbx::DevBuf<float> d_rs, d_ls;
  orbx::DevBuf<uint8_t> d_conn;
  // the per-live query scratch (flush grows it)
  int live_cap = 0;
  orbx::DevBuf<int32_t> d_live;
  orbx::DevBuf<unsigned long long> d_key, d_wkey;
  orbx::DevBuf<float> d_si, d_acc;
  orbx::DevBuf<int32_t> d_flag, d_best;
  orbx::DevBuf<long long> d_wid, d_cand;
  // the fixed blocks (orbx_kfdb_create)
  orbx::DevBuf<uint32_t> d_bitmap;
  orbx::DevBuf<orbx::KfCtl> d_ctl;
  orbx::DevBuf<uint32_t> d_qw;  // the host forms' query
  orbx::DevBuf<double> d_qv;
  orbx::DevBuf<int32_t> d_qn, d_ncand;
  int32_t h_qn = 0, h_ncand = 0;  // host ends of the two small copies: they outlive every early return
  // connected sets of the loop queries: pinned, read by the kernels in place
  orbx::PinnedBuf h_conn[orbx::kKfdbConnRing];
  orbx::Event conn_ev[orbx::kKfdbConnRing];
  bool conn_used[orbx::kKfdbConnRing] = {};
  int conn_next = 0;
};

namespace {

#define KF_CHECK(x)                             \
  do {                                          \
    if ((x) != hipSuccess) return ORBX_ERR_HIP; \
  } while (0)

// growth: the per-slot and per-live tables double from 1,024 entries, the pool holds twice what is asked
// for and at least 65,536 entries, a connected-set ring block twice the set and at least 256 slots
constexpr int table_slots(int n) { return 2 * n > 1024 ? 2 * n : 1024; }
constexpr long long pool_entries(long long n) { return 2 * n > (1 << 16) ? 2 * n : 1 << 16; }
constexpr size_t conn_slots(int n) { return 2 * n > 256 ? 2 * (size_t)n : 256; }

// a fresh array of new_n entries in place of *p, zeroed and/or holding the first old_n of the old one.  The
// fill and the copy go to st (the handle's own stream) and are waited for here, so whichever stream
// touches the array next finds them done, and only then is the new array swapped in; the caller has made
// sure nothing queued still reads *p (wait_queued).  On failure *p is untouched.
template <class T>
hipError_t grow(orbx::DevBuf<T>* p, size_t old_n, size_t new_n, bool keep, bool zero, hipStream_t st) {
  orbx::DevBuf<T> q;
  hipError_t e = q.ensure(new_n);
  if (e != hipSuccess) return e;
  const bool copy = keep && p->p && old_n;
  if (zero) e = hipMemsetAsync(q.p, 0, q.n * sizeof(T), st);
  if (e == hipSuccess && copy) e = hipMemcpyAsync(q.p, p->p, old_n * sizeof(T), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && (zero || copy)) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;  // (*p is still in place; q goes)
  p->swap(q);                     // the old array goes with q
  return hipSuccess;
}

// every queued query has run: the host may now move or free what they read
orbx_status wait_queued(orbx_kfdb* db) {
  if (db->ev_set) KF_CHECK(hipEventSynchronize(db->ev));
  return ORBX_OK;
}

// a slot for id (created with zeroed state when first seen); the per-slot tables grow by doubling
orbx_status slot_for(orbx_kfdb* db, long long id, int* out) {
  auto it = db->slot_of.find(id);
  if (it != db->slot_of.end()) {
    *out = it->second;
    return ORBX_OK;
  }
  const int s = (int)db->meta.size();
  if (s >= db->slot_cap) {
    const int oc = db->slot_cap, nc = table_slots(oc);
    KF_CHECK(grow(&db->d_meta, oc, nc, false, true, db->st));
    KF_CHECK(grow(&db->d_neigh, (size_t)oc * 10, (size_t)nc * 10, false, false, db->st));
    KF_CHECK(grow(&db->d_rq, oc, nc, true, true, db->st));
    KF_CHECK(grow(&db->d_lq, oc, nc, true, true, db->st));
    KF_CHECK(grow(&db->d_rw, oc, nc, true, true, db->st));
    KF_CHECK(grow(&db->d_lw, oc, nc, true, true, db->st));
    KF_CHECK(grow(&db->d_rs, oc, nc, true, true, db->st));
    KF_CHECK(grow(&db->d_ls, oc, nc, true, true, db->st));
    KF_CHECK(grow(&db->d_minkey, oc, nc, false, false, db->st));
    KF_CHECK(grow(&db->d_conn, oc, nc, false, true, db->st));
    db->slot_cap = nc;
    db->meta_lo = db->neigh_lo = 0;  // the mirrors are uploaded again in full
    db->meta_hi = db->neigh_hi = s;
  }
  KfMeta m{};
  m.id = id;
  db->meta.push_back(m);
  db->neigh.insert(db->neigh.end(), orbx::kKfdbNeigh, -1);
  db->live_pos.push_back(-1);
  db->slot_of.emplace(id, s);
  db->meta_lo = db->meta_hi > db->meta_lo ? std::min(db->meta_lo, s) : s;
  db->meta_hi = std::max(db->meta_hi, s + 1);
  db->neigh_lo = db->neigh_hi > db->neigh_lo ? std::min(db->neigh_lo, s) : s;
  db->neigh_hi = std::max(db->neigh_hi, s + 1);
  *out = s;
  return ORBX_OK;
}

void touch_meta(orbx_kfdb* db, int s) {
  db->meta_lo = db->meta_hi > db->meta_lo ? std::min(db->meta_lo, s) : s;
  db->meta_hi = std::max(db->meta_hi, s + 1);
}

// uploads what changed in the mirrors and sizes the per-query scratch, on stream s
orbx_status flush(orbx_kfdb* db, hipStream_t s) {
  if (db->meta_hi > db->meta_lo) {
    KF_CHECK(hipMemcpyAsync(db->d_meta.p + db->meta_lo, db->meta.data() + db->meta_lo,
                            sizeof(KfMeta) * (size_t)(db->meta_hi - db->meta_lo), hipMemcpyHostToDevice, s));
    db->meta_lo = db->meta_hi = 0;
  }
  if (db->neigh_hi > db->neigh_lo) {
    KF_CHECK(hipMemcpyAsync(db->d_neigh.p + (size_t)db->neigh_lo * 10, db->neigh.data() + (size_t)db->neigh_lo * 10,
                            40 * (size_t)(db->neigh_hi - db->neigh_lo), hipMemcpyHostToDevice, s));
    db->neigh_lo = db->neigh_hi = 0;
  }
  const int nl = (int)db->live.size();
  if (nl > db->live_cap) {  // only after an add, which waited for every queued query
    const int nc = table_slots(nl);
    KF_CHECK(grow(&db->d_live, 0, nc, false, false, db->st));
    KF_CHECK(grow(&db->d_key, 0, nc, false, false, db->st));
    KF_CHECK(grow(&db->d_wkey, 0, nc, false, false, db->st));
    KF_CHECK(grow(&db->d_si, 0, nc, false, false, db->st));
    KF_CHECK(grow(&db->d_acc, 0, nc, false, false, db->st));
    KF_CHECK(grow(&db->d_flag, 0, nc, false, false, db->st));
    KF_CHECK(grow(&db->d_best, 0, nc, false, false, db->st));
    KF_CHECK(grow(&db->d_wid, 0, nc, false, false, db->st));
    KF_CHECK(grow(&db->d_cand, 0, nc, false, false, db->st));
    db->live_cap = nc;
    db->live_dirty = true;
  }
  if (db->live_dirty && nl > 0)
    KF_CHECK(hipMemcpyAsync(db->d_live.p, db->live.data(), 4 * (size_t)nl, hipMemcpyHostToDevice, s));
  db->live_dirty = false;
  return ORBX_OK;
}

orbx::KfDev dev_view(const orbx_kfdb* db) {
  orbx::KfDev D{};
  D.words = db->d_words.p;
  D.vals = db->d_vals.p;
  D.meta = db->d_meta.p;
  D.live = db->d_live.p;
  D.n_live = (int)db->live.size();
  D.neigh = db->d_neigh.p;
  D.rq = db->d_rq.p;
  D.rw = db->d_rw.p;
  D.rs = db->d_rs.p;
  D.lq = db->d_lq.p;
  D.lw = db->d_lw.p;
  D.ls = db->d_ls.p;
  D.bitmap = db->d_bitmap.p;
  D.n_words = db->n_words;
  D.conn = db->d_conn.p;
  D.minkey = db->d_minkey.p;
  D.key = db->d_key.p;
  D.si = db->d_si.p;
  D.flag = db->d_flag.p;
  D.acc = db->d_acc.p;
  D.best = db->d_best.p;
  D.wkey = db->d_wkey.p;
  D.wid = db->d_wid.p;
  D.ctl = db->d_ctl.p;
  return D;
}

// moves the live entries into a fresh pool with room for `extra` more; add sequence numbers are
// renumbered 0.. in their order
orbx_status repool(orbx_kfdb* db, long long extra) {
  const int nl = (int)db->live.size();
  std::vector<int32_t> order(db->live);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return db->meta[a].seq < db->meta[b].seq; });
  std::vector<long long> new_off(std::max(nl, 1));
  long long used = 0;
  for (int i = 0; i < nl; i++) {
    new_off[i] = used;
    used += db->meta[order[i]].len;
  }
  const long long cap = pool_entries(used + extra);
  orbx::DevBuf<uint32_t> w1;
  orbx::DevBuf<double> v1;
  orbx::DevBuf<long long> d_off;
  orbx::DevBuf<int32_t> d_order;
  hipError_t e = w1.ensure((size_t)cap);
  if (e == hipSuccess) e = v1.ensure((size_t)cap);
  if (e == hipSuccess && nl > 0 && used > 0) {
    // the device still holds the old offsets: push pending mirror changes first
    orbx_status st = flush(db, db->st);
    if (st != ORBX_OK) e = hipErrorUnknown;
    if (e == hipSuccess) e = d_off.ensure((size_t)nl);
    if (e == hipSuccess) e = d_order.ensure((size_t)nl);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off.p, new_off.data(), 8 * (size_t)nl, hipMemcpyHostToDevice, db->st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_order.p, order.data(), 4 * (size_t)nl, hipMemcpyHostToDevice, db->st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(orbx::k_kfdb_compact, dim3(nl), dim3(256), 0, db->st, db->d_meta.p, d_order.p, d_off.p,
                         db->d_words.p, db->d_vals.p, w1.p, v1.p);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(db->st);
  }
  if (e != hipSuccess) return ORBX_ERR_HIP;
  db->d_words.swap(w1);  // (the old pool goes with w1, v1)
  db->d_vals.swap(v1);
  db->pool_cap = cap;
  db->pool_used = used;
  db->pool_dead = 0;
  for (int i = 0; i < nl; i++) {
    db->meta[order[i]].off = new_off[i];
    db->meta[order[i]].seq = (uint32_t)i;
    touch_meta(db, order[i]);
  }
  db->next_seq = (uint32_t)nl;
  return ORBX_OK;
}

bool query_ok(const uint32_t* words, const double* values, int n, unsigned n_words) {
  if (n < 0 || n > orbx::kKfdbMaxQuery || (n > 0 && (!words || !values))) return false;
  for (int i = 0; i < n; i++)
    if (words[i] >= n_words || (i && words[i] <= words[i - 1])) return false;
  return true;
}

hipStream_t pick_stream(orbx_kfdb* db, void* stream) {
  return stream == ORBX_STREAM_NULL ? (hipStream_t)0 : stream ? (hipStream_t)stream : db->st.st;
}

// queues one query on s: no host synchronisation (but see the connected-set ring)
orbx_status enqueue_query(orbx_kfdb* db, hipStream_t s, int loop, unsigned long long qid, const uint32_t* d_qw,
                          const double* d_qv, const int32_t* d_qn, const long long* connected, int n_connected,
                          float min_score, long long* d_cand, int cap, int32_t* d_ncand) {
  if (db->ev_set) KF_CHECK(hipStreamWaitEvent(s, db->ev, 0));  // queries run one after the other
  orbx_status fs = flush(db, s);
  if (fs != ORBX_OK) return fs;
  const int nl = (int)db->live.size();
  if (cap < 0) {  // the host forms: the handle's own list, one entry per live keyframe, the most there can be
    d_cand = db->d_cand.p;
    cap = db->live_cap;
  }
  if (nl == 0) {
    KF_CHECK(hipMemsetAsync(d_ncand, 0, 4, s));
  } else {
    orbx::KfQuery Q{};
    Q.words = d_qw;
    Q.vals = d_qv;
    Q.n = d_qn;
    Q.qid = qid;
    Q.loop = loop;
    Q.min_score = min_score;
    Q.cand = d_cand;
    Q.cap = cap;
    Q.n_cand = d_ncand;
    int ring = -1;
    if (loop && n_connected > 0) {
      ring = db->conn_next;
      db->conn_next = (ring + 1) % orbx::kKfdbConnRing;
      if (db->conn_used[ring]) KF_CHECK(hipEventSynchronize(db->conn_ev[ring]));  // its last reader is done
      orbx::PinnedBuf& block = db->h_conn[ring];
      if (4 * (size_t)n_connected > block.cap) KF_CHECK(block.ensure(4 * conn_slots(n_connected)));
      int32_t* const conn = block.as<int32_t>();
      int k = 0;
      for (int i = 0; i < n_connected; i++) {
        auto it = db->slot_of.find(connected[i]);
        if (it != db->slot_of.end()) conn[k++] = it->second;
      }
      Q.conn_list = conn;
      Q.n_conn = k;
    }
    const orbx::KfDev D = dev_view(db);
    const int per_live = (nl + 255) / 256;
    const int wide = std::max({per_live, orbx::kKfdbMaxQuery / 256, (Q.n_conn + 255) / 256});
    hipLaunchKernelGGL(orbx::k_kfdb_begin, dim3(wide), dim3(256), 0, s, D, Q);
    hipLaunchKernelGGL(orbx::k_kfdb_vote, dim3((nl + 3) / 4), dim3(256), 0, s, D, Q);
    hipLaunchKernelGGL(orbx::k_kfdb_commit, dim3(wide), dim3(256), 0, s, D, Q);
    hipLaunchKernelGGL(orbx::k_kfdb_acc, dim3(per_live), dim3(256), 0, s, D, Q);
    hipLaunchKernelGGL(orbx::k_kfdb_mark, dim3(per_live), dim3(256), 0, s, D);
    hipLaunchKernelGGL(orbx::k_kfdb_win, dim3(per_live), dim3(256), 0, s, D);
    hipLaunchKernelGGL(orbx::k_kfdb_rank, dim3(per_live), dim3(256), 0, s, D, Q);
    KF_CHECK(hipGetLastError());
    if (ring >= 0) {
      KF_CHECK(hipEventRecord(db->conn_ev[ring], s));
      db->conn_used[ring] = true;
    }
  }
  KF_CHECK(hipEventRecord(db->ev, s));
  db->ev_set = true;
  return ORBX_OK;
}

orbx_status host_query(orbx_kfdb* db, int loop, unsigned long long qid, const uint32_t* words, const double* values,
                       int n, const long long* connected, int n_connected, float min_score, long long* cand, int cap,
                       int* n_cand) {
  if (!db || !n_cand || cap < 0 || (cap > 0 && !cand) || n_connected < 0 || (n_connected > 0 && !connected))
    return ORBX_ERR_ARG;
  if (!query_ok(words, values, n, db->n_words)) return ORBX_ERR_ARG;
  KF_CHECK(hipSetDevice(db->device));
  db->h_qn = n;
  if (n > 0) {
    KF_CHECK(hipMemcpyAsync(db->d_qw.p, words, 4 * (size_t)n, hipMemcpyHostToDevice, db->st));
    KF_CHECK(hipMemcpyAsync(db->d_qv.p, values, 8 * (size_t)n, hipMemcpyHostToDevice, db->st));
  }
  hipError_t e = hipMemcpyAsync(db->d_qn.p, &db->h_qn, 4, hipMemcpyHostToDevice, db->st);
  orbx_status qs = e == hipSuccess ? enqueue_query(db, db->st, loop, qid, db->d_qw.p, db->d_qv.p, db->d_qn.p,
                                                   connected, n_connected, min_score, nullptr, -1, db->d_ncand.p)
                                   : ORBX_ERR_HIP;
  if (qs == ORBX_OK && hipMemcpyAsync(&db->h_ncand, db->d_ncand.p, 4, hipMemcpyDeviceToHost, db->st) != hipSuccess)
    qs = ORBX_ERR_HIP;
  // one synchronisation on every path: the caller's words / values are free again on return
  if (hipStreamSynchronize(db->st) != hipSuccess) qs = ORBX_ERR_HIP;
  if (qs != ORBX_OK) return qs;
  const int32_t m = db->h_ncand;
  *n_cand = m;
  if (m > cap) return ORBX_ERR_CAPACITY;
  if (m > 0) KF_CHECK(hipMemcpy(cand, db->d_cand.p, 8 * (size_t)m, hipMemcpyDeviceToHost));
  return ORBX_OK;
}

}  // namespace

extern "C" {

orbx_status orbx_kfdb_check_bow(const uint32_t* words, const double* values, int n, uint32_t n_words) {
  return query_ok(words, values, n, n_words) ? ORBX_OK : ORBX_ERR_ARG;
}

orbx_status orbx_kfdb_create(const orbx_voc* voc, int device, orbx_kfdb** out) {
  if (!out) return ORBX_ERR_ARG;
  *out = nullptr;
  if (device < 0) return ORBX_ERR_ARG;
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return ORBX_ERR_NODEV;
  if (!voc || device >= nd) return ORBX_ERR_ARG;
  int32_t info[6];
  if (orbx_voc_info(voc, info) != ORBX_OK) return ORBX_ERR_ARG;
  if (info[2] != 0 || info[5] < 0) return ORBX_ERR_ARG;  // L1 scoring only
  KF_CHECK(hipSetDevice(device));
  orbx_kfdb* db = new (std::nothrow) orbx_kfdb();
  if (!db) return ORBX_ERR_HIP;
  db->device = device;
  db->n_words = (unsigned)info[5];
  const size_t bm = ((size_t)db->n_words + 31) / 32 + 1;
  hipError_t e = db->st.ensure();
  if (e == hipSuccess) e = db->ev.ensure();
  for (int i = 0; i < orbx::kKfdbConnRing && e == hipSuccess; i++) e = db->conn_ev[i].ensure();
  if (e == hipSuccess) e = grow(&db->d_bitmap, 0, bm, false, true, db->st);
  if (e == hipSuccess) e = grow(&db->d_ctl, 0, 1, false, true, db->st);
  if (e == hipSuccess) e = grow(&db->d_qw, 0, orbx::kKfdbMaxQuery, false, true, db->st);
  if (e == hipSuccess) e = grow(&db->d_qv, 0, orbx::kKfdbMaxQuery, false, true, db->st);
  if (e == hipSuccess) e = grow(&db->d_qn, 0, 1, false, true, db->st);
  if (e == hipSuccess) e = grow(&db->d_ncand, 0, 1, false, true, db->st);
  if (e != hipSuccess) {
    orbx_kfdb_destroy(db);
    return ORBX_ERR_HIP;
  }
  *out = db;
  return ORBX_OK;
}

orbx_status orbx_kfdb_destroy(orbx_kfdb* db) {
  if (!db) return ORBX_ERR_ARG;
  (void)hipSetDevice(db->device);
  if (db->ev_set) (void)hipEventSynchronize(db->ev);
  if (db->st) (void)hipStreamSynchronize(db->st);
  delete db;
  return ORBX_OK;
}

orbx_status orbx_kfdb_add(orbx_kfdb* db, int64_t kf_id, const uint32_t* words, const double* values, int n) {
  if (!db || kf_id < 0) return ORBX_ERR_ARG;
  if (!query_ok(words, values, n, db->n_words)) return ORBX_ERR_ARG;
  {
    auto it = db->slot_of.find((long long)kf_id);
    if (it != db->slot_of.end() && db->meta[it->second].live) return ORBX_ERR_STATE;
  }
  KF_CHECK(hipSetDevice(db->device));
  orbx_status s = wait_queued(db);
  if (s != ORBX_OK) return s;
  int slot = -1;
  s = slot_for(db, (long long)kf_id, &slot);
  if (s != ORBX_OK) return s;
  if (db->pool_used + n > db->pool_cap || db->next_seq == 0xffffffffu) {
    s = repool(db, n);  // grows (and drops the dead entries on the way)
    if (s != ORBX_OK) return s;
  }
  if (n > 0) {
    KF_CHECK(hipMemcpyAsync(db->d_words.p + db->pool_used, words, 4 * (size_t)n, hipMemcpyHostToDevice, db->st));
    KF_CHECK(hipMemcpyAsync(db->d_vals.p + db->pool_used, values, 8 * (size_t)n, hipMemcpyHostToDevice, db->st));
    KF_CHECK(hipStreamSynchronize(db->st));  // the caller's arrays are free again on return
  }
  KfMeta& m = db->meta[slot];
  m.off = db->pool_used;
  m.len = n;
  m.seq = db->next_seq++;
  m.live = 1;
  db->pool_used += n;
  touch_meta(db, slot);
  db->live_pos[slot] = (int)db->live.size();
  db->live.push_back(slot);
  db->live_dirty = true;
  return ORBX_OK;
}

orbx_status orbx_kfdb_erase(orbx_kfdb* db, int64_t kf_id) {
  if (!db) return ORBX_ERR_ARG;
  auto it = db->slot_of.find((long long)kf_id);
  if (it == db->slot_of.end() || !db->meta[it->second].live) return ORBX_OK;  // the reference finds nothing to erase
  KF_CHECK(hipSetDevice(db->device));
  orbx_status s = wait_queued(db);
  if (s != ORBX_OK) return s;
  const int slot = it->second;
  KfMeta& m = db->meta[slot];
  m.live = 0;
  db->pool_dead += m.len;
  m.len = 0;
  touch_meta(db, slot);
  const int pos = db->live_pos[slot], last = db->live.back();
  db->live[pos] = last;
  db->live_pos[last] = pos;
  db->live.pop_back();
  db->live_pos[slot] = -1;
  db->live_dirty = true;
  if (db->live.empty()) {  // nothing left to move
    db->pool_used = db->pool_dead = 0;
    db->next_seq = 0;
    return ORBX_OK;
  }
  if (2 * db->pool_dead > db->pool_used) return repool(db, 0);  // more dead than live: compact
  return ORBX_OK;
}

orbx_status orbx_kfdb_clear(orbx_kfdb* db) {
  if (!db) return ORBX_ERR_ARG;
  KF_CHECK(hipSetDevice(db->device));
  orbx_status s = wait_queued(db);
  if (s != ORBX_OK) return s;
  const size_t nc = (size_t)db->slot_cap;
  if (nc) {
    KF_CHECK(hipMemsetAsync(db->d_rq.p, 0, 8 * nc, db->st));
    KF_CHECK(hipMemsetAsync(db->d_lq.p, 0, 8 * nc, db->st));
    KF_CHECK(hipMemsetAsync(db->d_rw.p, 0, 4 * nc, db->st));
    KF_CHECK(hipMemsetAsync(db->d_lw.p, 0, 4 * nc, db->st));
    KF_CHECK(hipMemsetAsync(db->d_rs.p, 0, 4 * nc, db->st));
    KF_CHECK(hipMemsetAsync(db->d_ls.p, 0, 4 * nc, db->st));
    KF_CHECK(hipStreamSynchronize(db->st));  // done before a query on any other stream can start
  }
  db->slot_of.clear();
  db->meta.clear();
  db->neigh.clear();
  db->live.clear();
  db->live_pos.clear();
  db->pool_used = db->pool_dead = 0;
  db->next_seq = 0;
  db->meta_lo = db->meta_hi = db->neigh_lo = db->neigh_hi = 0;
  db->live_dirty = false;
  return ORBX_OK;
}

orbx_status orbx_kfdb_set_neighbours(orbx_kfdb* db, const int64_t* kf_ids, const int64_t* best10,
                                     const int32_t* n_best, int n_kfs) {
  if (!db || n_kfs < 0 || (n_kfs > 0 && (!kf_ids || !best10 || !n_best))) return ORBX_ERR_ARG;
  for (int i = 0; i < n_kfs; i++) {
    if (kf_ids[i] < 0 || n_best[i] < 0 || n_best[i] > orbx::kKfdbNeigh) return ORBX_ERR_ARG;
    for (int j = 0; j < n_best[i]; j++)
      if (best10[(size_t)i * orbx::kKfdbNeigh + j] < 0) return ORBX_ERR_ARG;
  }
  if (n_kfs == 0) return ORBX_OK;
  KF_CHECK(hipSetDevice(db->device));
  orbx_status s = wait_queued(db);
  if (s != ORBX_OK) return s;
  for (int i = 0; i < n_kfs; i++) {
    int slot = -1;
    s = slot_for(db, (long long)kf_ids[i], &slot);
    if (s != ORBX_OK) return s;
    for (int j = 0; j < orbx::kKfdbNeigh; j++) {
      int nb = -1;
      if (j < n_best[i]) {
        s = slot_for(db, (long long)best10[(size_t)i * orbx::kKfdbNeigh + j], &nb);
        if (s != ORBX_OK) return s;
      }
      db->neigh[(size_t)slot * orbx::kKfdbNeigh + j] = nb;
    }
    db->neigh_lo = db->neigh_hi > db->neigh_lo ? std::min(db->neigh_lo, slot) : slot;
    db->neigh_hi = std::max(db->neigh_hi, slot + 1);
  }
  return ORBX_OK;
}

orbx_status orbx_kfdb_reloc_candidates(orbx_kfdb* db, uint64_t frame_id, const uint32_t* words, const double* values,
                                       int n, int64_t* cand, int cap, int* n_cand) {
  return host_query(db, 0, frame_id, words, values, n, nullptr, 0, 0.f, (long long*)cand, cap, n_cand);
}

orbx_status orbx_kfdb_loop_candidates(orbx_kfdb* db, uint64_t kf_mnid, const uint32_t* words, const double* values,
                                      int n, const int64_t* connected, int n_connected, float min_score,
                                      int64_t* cand, int cap, int* n_cand) {
  return host_query(db, 1, kf_mnid, words, values, n, (const long long*)connected, n_connected, min_score,
                    (long long*)cand, cap, n_cand);
}

orbx_status orbx_kfdb_reloc_candidates_device(orbx_kfdb* db, uint64_t frame_id, const uint32_t* d_words,
                                              const double* d_values, const int32_t* d_n, int64_t* d_cand, int cap,
                                              int32_t* d_n_cand, void* stream) {
  if (!db || !d_words || !d_values || !d_n || !d_n_cand || cap < 0 || (cap > 0 && !d_cand)) return ORBX_ERR_ARG;
  KF_CHECK(hipSetDevice(db->device));
  return enqueue_query(db, pick_stream(db, stream), 0, frame_id, d_words, d_values, d_n, nullptr, 0, 0.f,
                       (long long*)d_cand, cap, d_n_cand);
}

orbx_status orbx_kfdb_loop_candidates_device(orbx_kfdb* db, uint64_t kf_mnid, const uint32_t* d_words,
                                             const double* d_values, const int32_t* d_n, const int64_t* connected,
                                             int n_connected, float min_score, int64_t* d_cand, int cap,
                                             int32_t* d_n_cand, void* stream) {
  if (!db || !d_words || !d_values || !d_n || !d_n_cand || cap < 0 || (cap > 0 && !d_cand) || n_connected < 0 ||
      (n_connected > 0 && !connected))
    return ORBX_ERR_ARG;
  KF_CHECK(hipSetDevice(db->device));
  return enqueue_query(db, pick_stream(db, stream), 1, kf_mnid, d_words, d_values, d_n, (const long long*)connected,
                       n_connected, min_score, (long long*)d_cand, cap, d_n_cand);
}

orbx_status orbx_kfdb_score(orbx_kfdb* db, const uint32_t* words, const double* values, int n, const int64_t* kf_ids,
                            int n_kfs, double* scores) {
  if (!db || n_kfs < 0 || (n_kfs > 0 && (!kf_ids || !scores))) return ORBX_ERR_ARG;
  if (!query_ok(words, values, n, db->n_words)) return ORBX_ERR_ARG;
  std::vector<int32_t> slots(std::max(n_kfs, 1));
  for (int i = 0; i < n_kfs; i++) {
    auto it = db->slot_of.find((long long)kf_ids[i]);
    if (it == db->slot_of.end() || !db->meta[it->second].live) return ORBX_ERR_ARG;
    slots[i] = it->second;
  }
  if (n_kfs == 0) return ORBX_OK;
  KF_CHECK(hipSetDevice(db->device));
  hipStream_t s = db->st;
  if (db->ev_set) KF_CHECK(hipStreamWaitEvent(s, db->ev, 0));
  orbx_status fs = flush(db, s);
  if (fs != ORBX_OK) return fs;
  orbx::DevBuf<int32_t> d_slots;
  orbx::DevBuf<double> d_out;
  hipError_t e = d_slots.ensure((size_t)n_kfs);
  if (e == hipSuccess) e = d_out.ensure((size_t)n_kfs);
  db->h_qn = n;
  if (e == hipSuccess && n > 0) e = hipMemcpyAsync(db->d_qw.p, words, 4 * (size_t)n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && n > 0) e = hipMemcpyAsync(db->d_qv.p, values, 8 * (size_t)n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(db->d_qn.p, &db->h_qn, 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_slots.p, slots.data(), 4 * (size_t)n_kfs, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    const orbx::KfDev D = dev_view(db);
    const int qb = orbx::kKfdbMaxQuery / 256;
    hipLaunchKernelGGL(orbx::k_kfdb_bitmap, dim3(qb), dim3(256), 0, s, D.bitmap, D.n_words, db->d_qw.p, db->d_qn.p, 0);
    hipLaunchKernelGGL(orbx::k_kfdb_score, dim3((n_kfs + 3) / 4), dim3(256), 0, s, D, db->d_qw.p, db->d_qv.p,
                       db->d_qn.p, d_slots.p, n_kfs, d_out.p);
    hipLaunchKernelGGL(orbx::k_kfdb_bitmap, dim3(qb), dim3(256), 0, s, D.bitmap, D.n_words, db->d_qw.p, db->d_qn.p, 1);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(scores, d_out.p, 8 * (size_t)n_kfs, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  return (e == hipSuccess && e2 == hipSuccess) ? ORBX_OK : ORBX_ERR_HIP;
}

orbx_status orbx_kfdb_read_state(orbx_kfdb* db, const int64_t* kf_ids, int n, uint64_t* reloc_query,
                                 int32_t* reloc_words, float* reloc_score, uint64_t* loop_query, int32_t* loop_words,
                                 float* loop_score) {
  if (!db || n < 0 || (n > 0 && !kf_ids)) return ORBX_ERR_ARG;
  std::vector<int32_t> slots(std::max(n, 1));
  for (int i = 0; i < n; i++) {
    auto it = db->slot_of.find((long long)kf_ids[i]);
    if (it == db->slot_of.end()) return ORBX_ERR_ARG;  // never seen
    slots[i] = it->second;
  }
  if (n == 0) return ORBX_OK;
  KF_CHECK(hipSetDevice(db->device));
  orbx_status s = wait_queued(db);
  if (s != ORBX_OK) return s;
  const size_t ns = db->meta.size();
  std::vector<unsigned long long> q(ns);
  std::vector<int32_t> w(ns);
  std::vector<float> f(ns);
  if (reloc_query) {
    KF_CHECK(hipMemcpy(q.data(), db->d_rq.p, 8 * ns, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) reloc_query[i] = q[slots[i]];
  }
  if (loop_query) {
    KF_CHECK(hipMemcpy(q.data(), db->d_lq.p, 8 * ns, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) loop_query[i] = q[slots[i]];
  }
  if (reloc_words) {
    KF_CHECK(hipMemcpy(w.data(), db->d_rw.p, 4 * ns, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) reloc_words[i] = w[slots[i]];
  }
  if (loop_words) {
    KF_CHECK(hipMemcpy(w.data(), db->d_lw.p, 4 * ns, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) loop_words[i] = w[slots[i]];
  }
  if (reloc_score) {
    KF_CHECK(hipMemcpy(f.data(), db->d_rs.p, 4 * ns, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) reloc_score[i] = f[slots[i]];
  }
  if (loop_score) {
    KF_CHECK(hipMemcpy(f.data(), db->d_ls.p, 4 * ns, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) loop_score[i] = f[slots[i]];
  }
  return ORBX_OK;
}

orbx_status orbx_kfdb_size(const orbx_kfdb* db, int* live, long long* pool_entries) {
  if (!db) return ORBX_ERR_ARG;
  if (live) *live = (int)db->live.size();
  if (pool_entries) *pool_entries = db->pool_used;
  return ORBX_OK;
}

}  // extern "C"

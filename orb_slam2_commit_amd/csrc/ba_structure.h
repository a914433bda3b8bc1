// ba_structure.h -- LocalBundleAdjustment (localba.hip): the active-edge structure of a phase built
// on the device (k_ba_struct_count / _scan / _fill), problem intake (k_ba_prep), outlier marking
// between and after the phases (k_ba_outliers) and the result export (k_ba_export).
#pragma once
#include "ba_math.h"

namespace orbx {

// Block-wide exclusive scan of one int per thread under `op` (identity
// `ident`); *total gets the reduction over the block.  ws: NT/64 ints of LDS.
template <int NT, typename Op>
__device__ inline int ba_block_scan(int v, int ident, Op op, int* ws, int* total) {
  constexpr int NW = NT / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x = op(x, y);
  }
  if (lane == 63) ws[w] = x;
  __syncthreads();
  if (w == 0) {  // scan of the wave totals: NW lanes of wave 0
    int s = lane < NW ? ws[lane] : ident;
    for (int d = 1; d < NW; d <<= 1) {
      const int y = __shfl_up(s, d, 64);
      if (lane >= d) s = op(s, y);
    }
    if (lane < NW) ws[lane] = s;
  }
  __syncthreads();
  int ex = __shfl_up(x, 1, 64);
  if (lane == 0) ex = ident;
  const int r = w ? op(ws[w - 1], ex) : ex;
  *total = ws[NW - 1];
  __syncthreads();  // ws free for the next scan
  return r;
}

// Lanes of the wave holding the same key (keys < 2^nbits): one ballot per bit.
__device__ inline uint64_t ba_match(int key, int nbits) {
  uint64_t m = ~0ull;
  for (int b = 0; b < nbits; b++) {
    const bool s = (key >> b) & 1;
    const uint64_t bal = __ballot(s);
    m &= s ? bal : ~bal;
  }
  return m;
}

// Active-edge structure of a phase on the device: build_structure's one-pass
// (edges grouped by point) path, same arrays, same order, in three launches
// over tiles of kTileE edges (kTileT threads x kStructV contiguous edges, so
// positions keep edge order):
//  k_ba_struct_count  per tile: active edges per camera, active count,
//                     first/last active point, point segments inside the tile;
//  k_ba_struct_scan   one block: camera totals -> pose tables (one camera per
//                     thread, nc <= kStructMaxNc), per (tile, camera) cam_pos
//                     offsets, per tile position/point/segment carries, boff
//                     and the five sizes;
//  k_ba_struct_fill   per tile: act/pos_pt/pcam/pt_off/pt_id, and cam_pos as a
//                     stable per-wave multisplit of the tile's positions by
//                     camera (bitwise match, no atomics), ascending in a pose.
// 4 edges per thread (1,024-edge tiles): at config 4 the three launches take 23.7 µs against 29.5 with
// 8 (k_ba_struct_fill 14.5 -> 9.1, k_ba_struct_scan 8.7 -> 9.8 over twice the tiles; profiles/r05)
constexpr int kTileT = 256, kStructV = 4, kTileE = kTileT * kStructV;  // kTileE < 2^16: packed scans
constexpr int kStructNT = 1024, kStructMaxNc = 512, kStructMaxTiles = kStructNT;

__device__ inline void ba_tile_load(const BaDev& D, const uint8_t* __restrict__ flag, int lvl, int e0, bool* a,
                                    int* pt, int* cm) {
#pragma unroll
  for (int j = 0; j < kStructV; j++) {
    const int e = e0 + j;
    const bool in = e < D.ne;
    pt[j] = in ? D.ept[e] : -1;
    cm[j] = in ? D.ecam[e] : 0;
    a[j] = in && (lvl < 0 || flag[e] == lvl);
  }
}

struct BaAdd {
  __device__ int operator()(int a, int b) const { return a + b; }
};
struct BaMax {
  __device__ int operator()(int a, int b) const { return a > b ? a : b; }
};
struct BaMin {
  __device__ int operator()(int a, int b) const { return a < b ? a : b; }
};

__global__ __launch_bounds__(kTileT) void k_ba_struct_count(BaDev D, const uint8_t* __restrict__ flag, int lvl,
                                                            int* __restrict__ tcnt, int4* __restrict__ ttot) {
  if (spec_skip(D)) return;  // (block-uniform, before any barrier)
  constexpr int V = kStructV;
  extern __shared__ int sm_sc[];
  const int nc = D.nc, t = threadIdx.x, tile = blockIdx.x;
  int* hc = sm_sc;    // nc
  int* ws = hc + nc;  // kTileT/64
  for (int i = t; i < nc; i += kTileT) hc[i] = 0;
  bool a[V];
  int pt[V], cm[V];
  ba_tile_load(D, flag, lvl, tile * kTileE + t * V, a, pt, cm);
  __syncthreads();
  int nact = 0, lastp = -1, firstp = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < V; j++)
    if (a[j]) {
      atomicAdd(&hc[cm[j]], 1);
      nact++;
      lastp = pt[j];
      firstp = min(firstp, pt[j]);
    }
  int tlast, tot, tfirst;
  // points ascend along the edge list: the max over earlier edges is the
  // point of the last active edge before this thread's (-1: none in the tile)
  const int p = ba_block_scan<kTileT>(lastp, -1, BaMax(), ws, &tlast);
  int nseg = 0;
#pragma unroll
  for (int j = 0, q = p; j < V; j++)
    if (a[j]) {
      nseg += pt[j] != q;
      q = pt[j];
    }
  (void)ba_block_scan<kTileT>(nact | nseg << 16, 0, BaAdd(), ws, &tot);
  (void)ba_block_scan<kTileT>(firstp, 0x7fffffff, BaMin(), ws, &tfirst);
  for (int i = t; i < nc; i += kTileT) tcnt[(size_t)tile * nc + i] = hc[i];
  if (t == 0) ttot[tile] = make_int4(tot & 0xffff, tfirst, tlast, tot >> 16);
}

__global__ __launch_bounds__(kStructNT) void k_ba_struct_scan(BaDev D, const uint8_t* __restrict__ fixed, int ntiles,
                                                              int* __restrict__ tcnt, const int4* __restrict__ ttot,
                                                              int4* __restrict__ tcar, int* __restrict__ out) {
  if (spec_skip(D)) return;
  constexpr int NT = kStructNT;
  extern __shared__ int sm_ss[];
  const int nc = D.nc, t = threadIdx.x;
  int* coff = sm_ss;        // nposes+1
  int* ws = coff + nc + 1;  // NW
  // camera totals; tcnt becomes each tile's offset inside its camera's run
  int cc = 0;
  if (t < nc)
    for (int i0 = 0; i0 < ntiles; i0 += 8) {  // loads of 8 tiles in flight before their stores
      int x[8];
#pragma unroll
      for (int j = 0; j < 8; j++) x[j] = i0 + j < ntiles ? tcnt[(size_t)(i0 + j) * nc + t] : 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (i0 + j < ntiles) tcnt[(size_t)(i0 + j) * nc + t] = cc;
        cc += x[j];
      }
    }
  int nposes, tot, maxc, na, npa, nslots, tmp;
  const bool pose = t < nc && cc > 0 && !fixed[t];
  const int pidx = ba_block_scan<NT>(pose ? 1 : 0, 0, BaAdd(), ws, &nposes);
  const int pofs = ba_block_scan<NT>(pose ? cc : 0, 0, BaAdd(), ws, &tot);
  (void)ba_block_scan<NT>(pose ? cc : 0, 0, BaMax(), ws, &maxc);
  if (t < nc) D.chidx[t] = pose ? pidx : -1;
  if (pose) {
    D.pose_cam[pidx] = t;
    coff[pidx] = pofs;
    D.cam_off[pidx] = pofs;
  }
  // tile carries: first position, last active point before the tile, first segment
  const int4 tt = t < ntiles ? ttot[t] : make_int4(0, 0x7fffffff, -1, 0);
  const int kb = ba_block_scan<NT>(tt.x, 0, BaAdd(), ws, &na);
  const int pv = ba_block_scan<NT>(tt.z, -1, BaMax(), ws, &tmp);
  const int sg = tt.w - (tt.x > 0 && tt.y == pv ? 1 : 0);  // first point continues the previous tile's
  const int sb = ba_block_scan<NT>(sg, 0, BaAdd(), ws, &npa);
  if (t < ntiles) tcar[t] = make_int4(kb, pv, sb, 0);
  if (t == 0) {
    coff[nposes] = tot;
    D.cam_off[nposes] = tot;
    D.pt_off[npa] = na;
  }
  __syncthreads();
  // boff: block (c1, c2 >= c1) holds one slot per position of pose c1
  const int n1 = t < nposes ? coff[t + 1] - coff[t] : 0;
  const int q = ba_block_scan<NT>(t < nposes ? n1 * (nposes - t) : 0, 0, BaAdd(), ws, &nslots);
  if (t < nposes) {
    const int b0 = t * nposes - t * (t - 1) / 2;
    for (int j = 0; j < nposes - t; j++) D.boff[b0 + j] = q + j * n1;
  }
  if (t == 0) {
    D.boff[nposes * (nposes + 1) / 2] = nslots;
    out[0] = na;
    out[1] = npa;
    out[2] = nposes;
    out[3] = maxc;
    out[4] = nslots;
  }
}

__global__ __launch_bounds__(kTileT) void k_ba_struct_fill(BaDev D, const uint8_t* __restrict__ flag, int lvl,
                                                           const int* __restrict__ tcnt,
                                                           const int4* __restrict__ tcar) {
  if (spec_skip(D)) return;
  constexpr int V = kStructV, NW = kTileT / 64;
  extern __shared__ int sm_sf[];
  const int nc = D.nc, t = threadIdx.x, lane = t & 63, w = t >> 6, tile = blockIdx.x;
  int* chl = sm_sf;        // nc: pose index per camera
  int* cw = chl + nc;      // NW*nc: per-wave camera counts, then fill cursors
  int* lpc = cw + NW * nc; // kTileE: camera of each tile position (-1: fixed)
  int* ws = lpc + kTileE;  // NW
  for (int i = t; i < nc; i += kTileT) chl[i] = D.chidx[i];
  for (int i = t; i < NW * nc; i += kTileT) cw[i] = 0;
  const int4 car = tcar[tile];
  bool a[V];
  int pt[V], cm[V];
  const int e0 = tile * kTileE + t * V;
  ba_tile_load(D, flag, lvl, e0, a, pt, cm);
  int nact = 0, lastp = -1;
#pragma unroll
  for (int j = 0; j < V; j++) {
    nact += a[j];
    if (a[j]) lastp = pt[j];
  }
  int tlast, tks;
  int p = max(car.y, ba_block_scan<kTileT>(lastp, -1, BaMax(), ws, &tlast));
  int nseg = 0;
#pragma unroll
  for (int j = 0, q = p; j < V; j++)
    if (a[j]) {
      nseg += pt[j] != q;
      q = pt[j];
    }
  const int ks = ba_block_scan<kTileT>(nact | nseg << 16, 0, BaAdd(), ws, &tks);
  int kl = ks & 0xffff;
  int s = car.z + (ks >> 16) - 1;
#pragma unroll
  for (int j = 0; j < V; j++)
    if (a[j]) {
      if (pt[j] != p) {
        s++;
        D.pt_off[s] = car.x + kl;
        D.pt_id[s] = pt[j];
        p = pt[j];
      }
      const int pc = chl[cm[j]];
      D.act[car.x + kl] = e0 + j;
      D.pos_pt[car.x + kl] = s;
      D.pcam[car.x + kl] = pc;
      lpc[kl] = pc >= 0 ? cm[j] : -1;
      kl++;
    }
  __syncthreads();
  // cam_pos: stable multisplit of the tile's positions by camera
  const int nt = tks & 0xffff, nbits = 32 - __clz(nc);
  const int R = (((nt + NW - 1) / NW) + 63) & ~63;
  const int k0 = min(w * R, nt), k1 = min(k0 + R, nt);
  for (int kb = k0; kb < k1; kb += 64) {
    const int kk = kb + lane;
    const int c = kk < k1 ? lpc[kk] : -1;
    const uint64_t m = ba_match(c >= 0 ? c : nc, nbits);
    if (c >= 0 && __popcll(m & ((1ull << lane) - 1)) == 0) cw[w * nc + c] += __popcll(m);
  }
  __syncthreads();
  for (int c = t; c < nc; c += kTileT)
    if (chl[c] >= 0) {
      int run = D.cam_off[chl[c]] + tcnt[(size_t)tile * nc + c];
      for (int v = 0; v < NW; v++) {
        const int x = cw[v * nc + c];
        cw[v * nc + c] = run;
        run += x;
      }
    }
  __syncthreads();
  for (int kb = k0; kb < k1; kb += 64) {
    const int kk = kb + lane;
    const int c = kk < k1 ? lpc[kk] : -1;
    const uint64_t m = ba_match(c >= 0 ? c : nc, nbits);
    const int r = __popcll(m & ((1ull << lane) - 1));
    const int b = c >= 0 ? cw[w * nc + c] : 0;
    if (c >= 0) D.cam_pos[b + r] = car.x + kk;
    if (c >= 0 && r == 0) cw[w * nc + c] = b + __popcll(m);
  }
}

// Problem intake on the device: the caller's float observations / points
// become the FP64 edge and vertex arrays (Converter / g2o setMeasurement
// casts), the per-edge stereo flag, Huber delta (the float sqrt thresholds of
// src/Optimizer.cc:653-654, passed from the host) and its float square, robust
// flags on, stored errors zero.  Only the raw arrays cross PCIe.
__global__ __launch_bounds__(LBS) void k_ba_prep(int ne, int np, const float* __restrict__ obs,
                                                 const float* __restrict__ isig, const float* __restrict__ Xf,
                                                 double* __restrict__ X, uint8_t* __restrict__ est,
                                                 double* __restrict__ eobs, double* __restrict__ einfo,
                                                 double* __restrict__ edelta, float* __restrict__ edsqr,
                                                 uint8_t* __restrict__ erob, double* __restrict__ eerr, float thMono,
                                                 float thStereo) {
  const int i = blockIdx.x * LBS + threadIdx.x;
  if (i < ne) {
    const float u = obs[3 * i], v = obs[3 * i + 1], ur = obs[3 * i + 2];
    const bool s = ur >= 0;
    est[i] = s ? 1 : 0;
    eobs[3 * i] = u;
    eobs[3 * i + 1] = v;
    eobs[3 * i + 2] = ur;
    einfo[i] = isig[i];
    const double d = s ? thStereo : thMono;
    edelta[i] = d;
    edsqr[i] = (float)(d * d);
    erob[i] = 1;
    eerr[3 * i] = eerr[3 * i + 1] = eerr[3 * i + 2] = 0.0;
  }
  if (i < 3 * np) X[i] = Xf[i];
}

// phase transition (:764-802) and the final erase test (:817-847): per edge
// chi2 of its stored error against th, and depth of the current estimate
__global__ __launch_bounds__(LBS) void k_ba_outliers(BaDev D, uint8_t* flag, int drop_kernel) {
  if (spec_skip(D)) return;
  const int e = blockIdx.x * LBS + threadIdx.x;
  if (e >= D.ne) return;
  const int c = D.ecam[e], p = D.ept[e];
  const double info = D.einfo[e];
  double c2 = 0;
  const int Dm = D.est[e] ? 3 : 2;
  for (int i = 0; i < Dm; i++) c2 += D.eerr[3 * e + i] * (info * D.eerr[3 * e + i]);
  Quat q = {D.cq[4 * c], D.cq[4 * c + 1], D.cq[4 * c + 2], D.cq[4 * c + 3]};
  const double Xw[3] = {D.X[3 * p], D.X[3 * p + 1], D.X[3 * p + 2]};
  double Pc[3];
  qrot(q, Xw, Pc);
  const double z = Pc[2] + D.ct[3 * c + 2];
  const double th = D.est[e] ? 7.815 : 5.991;
  flag[e] = (c2 > th || !(z > 0.0)) ? 1 : 0;
  if (drop_kernel) D.erobust[e] = 0;
}

__global__ __launch_bounds__(LBS) void k_ba_export(BaDev D, float* Tcw, float* Xw, double* Tcw_d, double* Xw_d) {
  const int i = blockIdx.x * LBS + threadIdx.x;
  if (i < D.nc) {
    const Quat q = {D.cq[4 * i], D.cq[4 * i + 1], D.cq[4 * i + 2], D.cq[4 * i + 3]};
    double R[9];
    qmat(q, R);
    for (int r = 0; r < 3; r++) {
      for (int k = 0; k < 3; k++) {
        Tcw[12 * i + 4 * r + k] = (float)R[3 * r + k];
        if (Tcw_d) Tcw_d[12 * i + 4 * r + k] = R[3 * r + k];
      }
      Tcw[12 * i + 4 * r + 3] = (float)D.ct[3 * i + r];
      if (Tcw_d) Tcw_d[12 * i + 4 * r + 3] = D.ct[3 * i + r];
    }
  }
  if (i < D.np) {
    for (int r = 0; r < 3; r++) {
      Xw[3 * i + r] = (float)D.X[3 * i + r];
      if (Xw_d) Xw_d[3 * i + r] = D.X[3 * i + r];
    }
  }
}

}  // namespace orbx

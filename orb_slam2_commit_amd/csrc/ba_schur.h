// ba_schur.h -- LocalBundleAdjustment (localba.hip): the reduced camera system.  The per-phase pair
// table (k_ba_pair_table), the pair and rhs chunk partials (k_ba_pairs), their final sums
// (k_ba_schur_fin), and the fold flags of a device-LM trial (fused_mode, set_trial_folds).
#pragma once
#include "ba_linearize.h"

namespace orbx {

// Accumulates acc += BD_k1 Hpl_k2^T (6x3 * 3x6), one Hpl row at a time.
__device__ inline void pair_acc(double acc[36], const double A[18], const double* __restrict__ h2) {
#pragma unroll
  for (int c = 0; c < 6; c++) {
    const double b0 = h2[3 * c], b1 = h2[3 * c + 1], b2 = h2[3 * c + 2];
#pragma unroll
    for (int r = 0; r < 6; r++) acc[6 * r + c] += A[3 * r] * b0 + A[3 * r + 1] * b1 + A[3 * r + 2] * b2;
  }
}

__device__ inline int tri_decode(int b, int n, int& c1) {
  c1 = 0;
  while (b >= n - c1) {
    b -= n - c1;
    c1++;
  }
  return c1 + b;
}

// Once per phase (the structure is fixed across its LM trials): for Hschur
// block (c1, c2) and each position k1 of pose c1 (ascending, i.e. point
// order), the first position k2 of the same point on pose c2, flagged when
// the point has more than one.
// grid (nblk [+ the pblk blocks], chunks): blocks past nblk fill pblk (chunk 0 only)
__global__ __launch_bounds__(kPB) void k_ba_pair_table(BaDev D) {
  const int2 bxy = xcd_block2();  // (as k_ba_pairs: one pose chunk's blocks on one XCD)
  if (bxy.x >= D.nblk) {
    if (bxy.y == 0) pblk_body(D, bxy.x - D.nblk);
    return;
  }
  int c1;
  const int c2 = tri_decode(bxy.x, D.nposes, c1);
  int lo, hi;
  chunk_range(D.cam_off[c1], D.cam_off[c1 + 1], bxy.y, gridDim.y, lo, hi);
  int* tab = D.ptab + D.boff[bxy.x] - D.cam_off[c1];
  for (int t = lo + threadIdx.x; t < hi; t += kPB) {
    const int i = D.pos_pt[D.cam_pos[t]];
    const int s = D.pt_off[i], e = D.pt_off[i + 1];
    int first = -1, more = 0;
    for (int k0 = s; k0 < e; k0 += 8) {  // the point's pose indices, eight loads in flight (clamped)
      int pc[8];
#pragma unroll
      for (int u = 0; u < 8; u++) pc[u] = D.pcam[min(k0 + u, e - 1)];
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (k0 + u < e && pc[u] == c2) {
          more |= first >= 0;
          first = first < 0 ? k0 + u : first;
        }
    }
    tab[t] = first < 0 ? -1 : (first | (more << 30));
  }
}

// device-LM value of BaDev::fused: 2 = k_ba_lin_schur also takes the non-relinearising trials'
// point side and k_ba_point_schur is not launched.  A problem without free poses keeps 1
// (k_ba_point_schur flags its empty reduced system).
static int fused_mode(int nbf, int nposes) {
  if (nbf <= 0) return 0;
  return nposes > 0 ? 2 : 1;
}
// The device-LM trial copy's fold flags (single and batched drivers alike, so a batched problem
// keeps its single run's bits): with k_ba_lin_schur doing every trial's point side (fused == 2),
// B D^-1 is formed inside k_ba_pairs (bdfold) and, where the per-block pose records fit
// (gpose allocated: at most kPosePartMaxPoses poses and kPosePartMaxDoubles doubles), the pose
// terms leave k_ba_lin_schur summed per block and pose (posepart).
constexpr size_t kPosePartMaxDoubles = 1 << 22;  // nbf x nposes x kCmc (32 MB)
__host__ inline void set_trial_folds(BaDev& d) {
  d.bdfold = d.fused == 2 ? 1 : 0;
  d.posepart = (d.fused == 2 && d.gpose) ? 1 : 0;
}

// pose-term chunk partials of a camfold trial, after the pair and rhs partials
__device__ inline size_t cam_part_off(const BaDev& D) { return ((size_t)D.nblk * 36 + (size_t)D.nposes * 6) * D.gsplit; }

// Grid (nblk + nposes, chunk).  Blocks b < nblk: Hschur block (c1 <= c2)
// pair sum  sum BD_k1 Hpl_k2^T  over the pairs of k_ba_pair_table; thread t of
// a chunk takes pose c1's positions t, t+kPB, ... (each thread's pairs in
// (k1, k2) order).  Blocks b >= nblk: sum of cf over pose b - nblk's positions
// (the Schur rhs correction).  Chunk partials -> gpart; k_ba_schur_fin sums
// them in chunk order (deterministic).
// device-LM trials fold k_ba_cam_sum / k_ba_cam_fin into k_ba_pairs / k_ba_schur_fin (the entry
// linearisation of a phase still launches them)
// (gx, gy) = the block's (Hschur / rhs block, chunk) in the launch grid, taken XCD-contiguous
// (xcd_block2): the Hschur blocks of one (c1, chunk) share an XCD, so chunk c1's BD rows come from
// one L2 -- 50.7 -> 24.3 MB fetched per launch, 20.0 -> 18.9 us at config 4 (profiles/r05)
__device__ __forceinline__ void k_ba_pairs_body(const BaDev& D, int gx, int gy) {
  if (lm_skip(D) || gx >= D.nblk + D.nposes || gy >= D.gsplit) return;
  __shared__ double red[(kPB / 64 + 1) * 36];
  const int S = D.gsplit, s = gy;
  // dispatch order: the rhs blocks (every position of a pose, the pose terms too) first, then the
  // Schur blocks -- the heaviest blocks leave first and the grid's second round is light ones
  const int bx = gx < D.nposes ? D.nblk + gx : gx - D.nposes;
  if (bx >= D.nblk) {
    const int ci = bx - D.nblk;
    const bool cam = D.camfold && !lm_skip_lin(D);  // block-uniform
    double v[6] = {0, 0, 0, 0, 0, 0};
    double w[27];
#pragma unroll
    for (int j = 0; j < 27; j++) w[j] = 0;
    int lo, hi;
    chunk_range(D.cam_off[ci], D.cam_off[ci + 1], s, S, lo, hi);
    const bool camp = cam && !D.posepart;
    for (int t = lo + threadIdx.x; t < hi; t += kPB) {
      const int k = D.cam_pos[t];
      const double* f = D.cf + 6 * (size_t)k;
#pragma unroll
      for (int r = 0; r < 6; r++) v[r] += f[r];
      if (camp) {  // k_ba_cam_sum's accumulation (same chunks, same per-thread positions)
        const double* cm = D.cmc + kCmc * (size_t)k;
#pragma unroll
        for (int j = 0; j < kCmc; j++) w[j] += cm[j];
      }
    }
    if (cam && D.posepart) {  // the fused blocks' per-pose sums, chunked over the blocks
      int blo, bhi;
      chunk_range(0, D.nbf, s, S, blo, bhi);
      for (int b = blo + threadIdx.x; b < bhi; b += kPB) {
        const double* g = D.gpose + ((size_t)b * D.nposes + ci) * kCmc;
#pragma unroll
        for (int j = 0; j < kCmc; j++) w[j] += g[j];
      }
    }
    const double* tot = block_sum_fixed<6, kPB / 64>(v, red);
    if (threadIdx.x < 6)
      D.gpart[(size_t)D.nblk * S * 36 + ((size_t)ci * S + s) * 6 + threadIdx.x] = tot[threadIdx.x];
    if (cam) {
      static_assert(kPB == kGB, "k_ba_cam_sum's block shape");
      __syncthreads();  // red is reused
      const double* tc = block_sum_fixed<27, kPB / 64>(w, red);
      if (threadIdx.x < 27) D.gpart[cam_part_off(D) + ((size_t)ci * S + s) * 27 + threadIdx.x] = tc[threadIdx.x];
    }
    return;
  }
  int c1;
  const int c2 = tri_decode(bx, D.nposes, c1);
  double acc[36];
#pragma unroll
  for (int j = 0; j < 36; j++) acc[j] = 0;
  int lo, hi;
  chunk_range(D.cam_off[c1], D.cam_off[c1 + 1], s, S, lo, hi);
  const int* tab = D.ptab + D.boff[bx] - D.cam_off[c1];
  for (int t = lo + threadIdx.x; t < hi; t += kPB) {
    const int v = tab[t];
    const int k1 = D.cam_pos[t];
    if (v < 0) continue;
    const int first = v & ((1 << 30) - 1);
    double A[18];
    if (D.bdfold) {  // B D^-1 = H_pl D^-1 of the point (k_ba_lin_schur's expression, the same bits)
      const double* B1 = D.Hpl + 18 * (size_t)k1;
      const double* Di = D.Dinv + 9 * (size_t)D.pos_pt[k1];
      double h[18], di[9];
#pragma unroll
      for (int j = 0; j < 18; j++) h[j] = B1[j];
#pragma unroll
      for (int j = 0; j < 9; j++) di[j] = Di[j];
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) A[3 * r + c] = h[3 * r] * di[c] + h[3 * r + 1] * di[3 + c] + h[3 * r + 2] * di[6 + c];
    } else {
      const double* bd = D.BD + 18 * (size_t)k1;
#pragma unroll
      for (int j = 0; j < 18; j++) A[j] = bd[j];
    }
    pair_acc(acc, A, D.Hpl + 18 * (size_t)first);
    if (v >> 30) {
      const int e = D.pt_off[D.pos_pt[k1] + 1];
      for (int k2 = first + 1; k2 < e; k2++)
        if (D.pcam[k2] == c2) pair_acc(acc, A, D.Hpl + 18 * (size_t)k2);
    }
  }
  const double* tot = block_sum_fixed<36, kPB / 64>(acc, red);
  if (threadIdx.x < 36) D.gpart[((size_t)bx * S + s) * 36 + threadIdx.x] = tot[threadIdx.x];
}
__global__ __launch_bounds__(kPB) void k_ba_pairs(BaDev D) {
  const int2 b = xcd_block2();
  k_ba_pairs_body(D, b.x, b.y);
}
__global__ __launch_bounds__(kPB) void k_ba_pairs_many(const BaDev* __restrict__ Ds) {
  const int3 b = xcd_block3();
  k_ba_pairs_body(Ds[b.z], b.x, b.y);
}

// Reduced system from the chunk partials: blocks b < nblk write Hschur block
// (c1, c2) = [c1==c2](Hpp + lambda I) - pair sum (both triangles, so every
// entry of S is written); blocks b >= nblk write bs = bp - sum cf.
__device__ inline void schur_fin_block(const BaDev& D, int blk, int j, double lambda) {
  const int S = D.gsplit;
  // sum of the S chunk partials at p, p + stride, ... in chunk order; loads issued in groups of 8
  // (clamped, not predicated) before their adds
  auto psum = [&](const double* p, size_t stride) {
    double t = 0;
    for (int c0 = 0; c0 < S; c0 += 8) {
      double v[8];
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const double* q = p + (size_t)min(c0 + e, S - 1) * stride;
        v[e] = *q;
      }
#pragma unroll
      for (int e = 0; e < 8; e++)
        if (c0 + e < S) t += v[e];
    }
    return t;
  };
  const bool cam = D.camfold && !lm_skip_lin(D);  // k_ba_cam_fin's sums (chunk order) done here
  const double* camp = D.gpart + cam_part_off(D);
  if (blk >= D.nblk) {
    const int ci = blk - D.nblk;
    if (j < 6) {
      const double t = psum(D.gpart + (size_t)D.nblk * S * 36 + (size_t)ci * S * 6 + j, 6);
      double bp;
      if (cam) {
        bp = psum(camp + (size_t)ci * S * 27 + 21 + j, 27);
        D.bp[6 * ci + j] = bp;
      } else {
        bp = D.bp[6 * ci + j];
      }
      D.bs[6 * ci + j] = bp - t;
    }
    return;
  }
  if (j >= 36) return;
  int c1;
  const int c2 = tri_decode(blk, D.nposes, c1);
  const double v = psum(D.gpart + (size_t)blk * S * 36 + j, 36);
  const int N = 6 * D.nposes;
  const int r = j / 6, c = j % 6;
  double sv;
  if (c1 == c2) {
    double h;
    if (cam) {
      const int lo = min(r, c), hi = max(r, c);
      h = psum(camp + (size_t)c1 * S * 27 + lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo), 27);
      D.Hpp[36 * c1 + j] = h;
    } else {
      h = D.Hpp[36 * c1 + j];
    }
    sv = h + (r == c ? lambda : 0.0) - v;
  } else {
    sv = -v;
    D.S[(size_t)(6 * c2 + c) * N + 6 * c1 + r] = sv;
  }
  D.S[(size_t)(6 * c1 + r) * N + 6 * c2 + c] = sv;
}
__device__ __forceinline__ void k_ba_schur_fin_body(const BaDev& D, double lambda) {
  if (lm_skip(D) || (int)blockIdx.x >= D.nblk + D.nposes) return;
  schur_fin_block(D, blockIdx.x, threadIdx.x, lm_lambda(D, lambda));
}
__global__ __launch_bounds__(64) void k_ba_schur_fin(BaDev D, double lambda) { k_ba_schur_fin_body(D, lambda); }
__global__ __launch_bounds__(64) void k_ba_schur_fin_many(const BaDev* __restrict__ Ds, double lambda) {
  k_ba_schur_fin_body(Ds[blockIdx.z], lambda);
}

}  // namespace orbx

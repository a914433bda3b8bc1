// mapping.hip -- the two small per-MapPoint / per-KeyFrame routines of
// SURVEY §8(f) row 4, batched:
//
//   k_distinctive  MapPoint::ComputeDistinctiveDescriptors  src/MapPoint.cc:249-320
//   k_undistort    Frame::UndistortKeyPoints               src/Frame.cc:471-506
//                  (cv::undistortPoints, OpenCV 3.2 cvUndistortPoints)
//
// k_distinctive: one wave per MapPoint.  The reference builds the N x N
// Hamming matrix, sorts every row and keeps the first row with the smallest
// vDists[(size_t)(0.5*(N-1))].  Here lane i owns row i and finds that order
// statistic without storing or sorting the row: the k-th smallest of N
// integers in [0,256] is the largest t with #{j : d(i,j) < t} <= k, built bit
// by bit in 9 counting passes over the point's descriptors (wave-uniform
// addresses, so the descriptor loads are scalar and shared by all lanes).
// The row winner is a wave min over (median << 16 | i): smallest median,
// first row on ties, as the reference's strict `median < BestMedian`.
// Bytes per point: 32 N read (L1/K$-resident after the first pass), 36 written.
//
// k_undistort: one thread per keypoint over undistort_keypoint (orbx_undistort.h: all FP64 in
// cvUndistortPoints' operation order), so keys_un equals the oracle bit for bit.  28 B read + 28 B
// written per keypoint: HBM-bound when batched.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <vector>

#include "orbx_scratch.h"
#include "orbx_device.h"
#include "orbx_internal.h"
#include "orbx_undistort.h"

namespace orbx {
namespace mapping {

constexpr int MBS = 256;  // 4 MapPoints per block
constexpr int UBS = 256;

__global__ __launch_bounds__(MBS) void k_distinctive(const uint8_t* __restrict__ desc,
                                                     const int32_t* __restrict__ obs_off, int n_points,
                                                     int32_t* __restrict__ best, uint8_t* __restrict__ out_desc) {
  const int lane = threadIdx.x & 63;
  const int p = __builtin_amdgcn_readfirstlane(blockIdx.x * (MBS / 64) + (threadIdx.x >> 6));
  if (p >= n_points) return;  // whole wave
  const int o0 = obs_off[p], n = obs_off[p + 1] - o0;
  if (n <= 0) {
    if (lane == 0) best[p] = -1;
    return;
  }
  const uint64_t* D = (const uint64_t*)(desc + (size_t)o0 * 32);
  const int k = (n - 1) >> 1;  // (size_t)(0.5*(N-1)), src/MapPoint.cc:306
  uint32_t key = 0xFFFFFFFFu;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    uint64_t di[4] = {0, 0, 0, 0};
    if (i < n) {
      di[0] = D[4 * i];
      di[1] = D[4 * i + 1];
      di[2] = D[4 * i + 2];
      di[3] = D[4 * i + 3];
    }
    int t = 0;  // largest t with #{d < t} <= k  ==  the k-th smallest distance of row i
#pragma unroll 1
    for (int b = 256; b > 0; b >>= 1) {
      const int c = t + b;
      int cnt = 0;
      for (int j = 0; j < n; j++) cnt += hamming256(di, D + 4 * j) < c;
      if (cnt <= k) t = c;
    }
    if (i < n) {
      const uint32_t kk = ((uint32_t)t << 16) | (uint32_t)i;
      key = kk < key ? kk : key;
    }
  }
  key = wave_min_u32(key);
  const int bi = (int)(key & 0xFFFF);
  if (lane == 0) best[p] = bi;
  if (out_desc && lane < 8)
    ((uint32_t*)(out_desc + (size_t)p * 32))[lane] = ((const uint32_t*)(desc + ((size_t)o0 + bi) * 32))[lane];
}

__global__ __launch_bounds__(UBS) void k_undistort(const orbx_keypoint* __restrict__ keys,
                                                   const int32_t* __restrict__ frame_off,
                                                   const orbx_camera* __restrict__ cams,
                                                   orbx_keypoint* __restrict__ keys_un) {
  const int f = blockIdx.y;
  const int a = frame_off[f], n = frame_off[f + 1] - a;
  const int i = blockIdx.x * UBS + threadIdx.x;
  if (i >= n) return;
  orbx_keypoint kp = keys[a + i];
  const orbx_camera& cam = cams[f];
  undistort_keypoint(cam, kp);  // a plain copy when mDistCoef.at<float>(0)==0.0 (src/Frame.cc:474-478)
  keys_un[a + i] = kp;
}

}  // namespace mapping
}  // namespace orbx

// ------------------------------------------------------------------ C ABI
using orbx::camera_ok;

extern "C" orbx_status orbx_distinctive_descriptors_device(const uint8_t* desc, const int32_t* obs_off, int n_points,
                                                           int32_t* best, uint8_t* out_desc, void* stream) {
  if (n_points < 0 || (n_points > 0 && (!desc || !obs_off || !best))) return ORBX_ERR_ARG;
  if (n_points == 0) return ORBX_OK;
  const int grid = (n_points + orbx::mapping::MBS / 64 - 1) / (orbx::mapping::MBS / 64);
  hipLaunchKernelGGL(orbx::mapping::k_distinctive, dim3(grid), dim3(orbx::mapping::MBS), 0, (hipStream_t)stream,
                     desc, obs_off, n_points, best, out_desc);
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_HIP;
}

extern "C" orbx_status orbx_distinctive_descriptors(const uint8_t* desc, const int32_t* obs_off, int n_points,
                                                    int32_t* best, uint8_t* out_desc, int device) {
  if (n_points < 0 || (n_points > 0 && (!desc || !obs_off || !best))) return ORBX_ERR_ARG;
  if (n_points == 0) return ORBX_OK;
  if (obs_off[0] != 0) return ORBX_ERR_ARG;
  for (int p = 0; p < n_points; p++)  // host check of the CSR the kernel trusts (row index fits 16 bits)
    if (obs_off[p + 1] < obs_off[p] || obs_off[p + 1] - obs_off[p] > 65535) return ORBX_ERR_ARG;
  const orbx_status ds = orbx::select_device(device);
  if (ds != ORBX_OK) return ds;
  using orbx::Staging;
  const size_t nd = (size_t)obs_off[n_points], np = (size_t)n_points;
  Staging S(device);
  const auto s_desc = S.in(desc, nd * 32);
  const auto s_off = S.in(obs_off, np + 1);
  const auto s_best = S.out<int32_t>(np);
  const auto s_out = S.out<uint8_t>(out_desc ? np * 32 : 0);
  orbx_status st = S.commit();
  if (st != ORBX_OK) return st;
  hipError_t e = S.upload(Staging::Outputs::skipped);
  if (e != hipSuccess) return ORBX_ERR_HIP;
  st = orbx_distinctive_descriptors_device(S.dev(s_desc), S.dev(s_off), n_points, S.dev(s_best),
                                           out_desc ? S.dev(s_out) : nullptr, S.stream());
  if (st != ORBX_OK) return st;
  e = S.download();
  if (e == hipSuccess) e = S.sync();
  if (e != hipSuccess) return ORBX_ERR_HIP;
  S.fetch(s_best, best, np);
  S.fetch(s_out, out_desc, np * 32);
  return ORBX_OK;
}

extern "C" orbx_status orbx_undistort_keypoints_device(const orbx_keypoint* keys, const int32_t* frame_off,
                                                       int n_frames, int max_keys, const orbx_camera* cams,
                                                       orbx_keypoint* keys_un, void* stream) {
  if (n_frames < 0 || max_keys < 0 || (n_frames > 0 && (!keys || !frame_off || !cams || !keys_un)))
    return ORBX_ERR_ARG;
  if (n_frames == 0 || max_keys == 0) return ORBX_OK;
  if (n_frames > 65535) return ORBX_ERR_SIZE;
  const dim3 grid((max_keys + orbx::mapping::UBS - 1) / orbx::mapping::UBS, n_frames);
  hipLaunchKernelGGL(orbx::mapping::k_undistort, grid, dim3(orbx::mapping::UBS), 0, (hipStream_t)stream, keys,
                     frame_off, cams, keys_un);
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_HIP;
}

extern "C" orbx_status orbx_undistort_keypoints(const orbx_keypoint* keys, int n, const orbx_camera* cam,
                                                orbx_keypoint* keys_un, int device) {
  if (n < 0 || !cam || (n > 0 && (!keys || !keys_un))) return ORBX_ERR_ARG;
  if (!camera_ok(*cam)) return ORBX_ERR_ARG;
  if (n == 0) return ORBX_OK;
  const orbx_status ds = orbx::select_device(device);
  if (ds != ORBX_OK) return ds;
  using orbx::Staging;
  const int32_t off[2] = {0, n};
  Staging S(device);
  const auto s_in = S.in(keys, (size_t)n);
  const auto s_off = S.in(off, 2);
  const auto s_cam = S.in(cam, 1);
  const auto s_out = S.out<orbx_keypoint>((size_t)n);
  orbx_status st = S.commit();
  if (st != ORBX_OK) return st;
  hipError_t e = S.upload(Staging::Outputs::skipped);
  if (e != hipSuccess) return ORBX_ERR_HIP;
  st = orbx_undistort_keypoints_device(S.dev(s_in), S.dev(s_off), 1, n, S.dev(s_cam), S.dev(s_out), S.stream());
  if (st != ORBX_OK) return st;
  e = S.download();
  if (e == hipSuccess) e = S.sync();
  if (e != hipSuccess) return ORBX_ERR_HIP;
  S.fetch(s_out, keys_un, (size_t)n);
  return ORBX_OK;
}

// rgbd.hip -- the RGB-D front end: what Tracking::GrabImage* and Frame's RGB-D constructor do to a
// frame around the ORB extraction.
//
//   k_cvt_gray     cv::cvtColor 8U, 3 or 4 channels -> 1     src/Tracking.cc:174-199, 215-228, 246-259
//                  (OpenCV 3.2 RGB2Gray<uchar>)
//   k_rgbd_finish  Frame::UndistortKeyPoints + ComputeStereoFromRGBD + the per-pixel part of
//                  imDepth.convertTo(CV_32F, mDepthMapFactor)   src/Frame.cc:471-506, 791-816,
//                                                               src/Tracking.cc:230-231
//
// k_cvt_gray is a pure streaming kernel: (C + 1) bytes per pixel, no reuse.  A lane owns four
// output pixels, i.e. one aligned dword of the grey row, and the 4C source bytes under them.  The
// source bytes of a 3-byte pixel are never dword-aligned and a row may start anywhere (the pitch
// is the caller's), so a lane loads the C or C + 1 ALIGNED dwords that cover its span and shifts
// its bytes out of neighbouring pairs with v_alignbyte; neighbouring lanes' spans are adjacent, so
// a wave reads one contiguous run of 64 * 4C bytes.  No byte loads anywhere: the head (the 0-3
// pixels before the grey row's first aligned dword) and the tail (the 0-3 after its last) take the
// same aligned loads per pixel and store bytes.  A loaded dword always holds at least one byte of
// the row, so nothing outside the row's own aligned words is touched.
//
//   Y = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14
// is RGB2Gray<uchar>'s table form (R2Y, G2Y, B2Y at yuv_shift = 14, the rounding constant folded
// into one table); alpha is ignored.
//
// k_rgbd_finish: one block per frame, a thread per keypoint.  The depth image is only ever read
// under the keypoints (src/Frame.cc:806), so the conversion convertTo would apply to the whole
// image is applied at the lookup: N reads instead of a W x H float image.
#include <hip/hip_runtime.h>

#include "orbx_device.h"
#include "orbx_rgbd.h"
#include "orbx_undistort.h"

namespace orbx {
namespace {

constexpr int kGrayBX = 64, kGrayBY = 4;  // k_cvt_gray block: one wave along a row, four rows
constexpr int kFinishBS = 1024;

__device__ __forceinline__ uint32_t gray_of(uint32_t b0, uint32_t b1, uint32_t b2, int c0, int c2) {
  return (b0 * (uint32_t)c0 + b1 * (uint32_t)kG2Y + b2 * (uint32_t)c2 + (1u << (kYuvShift - 1))) >> kYuvShift;
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t* p, int k) { return (p[k >> 2] >> (8 * (k & 3))) & 255u; }

template <int C>
__global__ __launch_bounds__(kGrayBX* kGrayBY) void k_cvt_gray(CvtGrayArgs A) {
  const int y = blockIdx.y * kGrayBY + threadIdx.y, img = blockIdx.z;
  if (y >= A.h) return;
  const uint8_t* srow = A.src + (long long)img * A.src_image_pitch + (long long)y * A.src_pitch;
  uint8_t* drow = A.dst + (long long)img * A.dst_image_pitch + (long long)y * A.dst_pitch;
  // item 0: the head, pixels [0, head); item j >= 1: the four pixels of one aligned dword of the
  // grey row (fewer at the row's end: the tail)
  const int head = min((int)((0 - (uintptr_t)drow) & 3), A.w);
  const int j = blockIdx.x * kGrayBX + threadIdx.x;
  const int x0 = j == 0 ? 0 : head + 4 * (j - 1);
  const int cnt = j == 0 ? head : min(4, A.w - x0);
  if (cnt <= 0) return;
  if (cnt == 4) {
    const uint8_t* a = srow + (long long)C * x0;
    const int s = (int)((uintptr_t)a & 3);
    const uint32_t* base = (const uint32_t*)(a - s);
    uint32_t w[C + 1];
#pragma unroll
    for (int k = 0; k < C; k++) w[k] = __builtin_nontemporal_load(base + k);
    w[C] = s ? __builtin_nontemporal_load(base + C) : 0u;  // bytes of the span reach into it only then
    uint32_t p[C];
#pragma unroll
    for (int k = 0; k < C; k++) p[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], (uint32_t)s);
    uint32_t out = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
      out |= gray_of(byte_of(p, C * q), byte_of(p, C * q + 1), byte_of(p, C * q + 2), A.c0, A.c2) << (8 * q);
    *(uint32_t*)(drow + x0) = out;
    return;
  }
  for (int q = 0; q < cnt; q++) {
    const uint8_t* a = srow + (long long)C * (x0 + q);
    const int s = (int)((uintptr_t)a & 3);
    const uint32_t* base = (const uint32_t*)(a - s);
    const uint32_t w0 = __builtin_nontemporal_load(base);
    const uint32_t w1 = s + C > 4 ? __builtin_nontemporal_load(base + 1) : 0u;
    const uint32_t p = __builtin_amdgcn_alignbyte(w1, w0, (uint32_t)s);
    drow[x0 + q] = (uint8_t)gray_of(p & 255u, (p >> 8) & 255u, (p >> 16) & 255u, A.c0, A.c2);
  }
}

__global__ __launch_bounds__(kFinishBS) void k_rgbd_finish(RgbdFinishArgs A) {
  __shared__ int s_sum[2];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = min(A.counts[(long long)f * A.n_stride], A.max_k);
  if (tid < 2) s_sum[tid] = 0;
  __syncthreads();
  const orbx_keypoint* kps = A.kps + (long long)f * A.k_stride;
  orbx_keypoint* kun = A.kps_un + (long long)f * A.k_stride;
  float* uR = A.uR + (long long)f * A.out_stride;
  float* dep = A.dep + (long long)f * A.out_stride;
  const uint8_t* img = A.depth + (long long)f * A.depth_image_pitch;
  int pos = 0, oob = 0;
  for (int i = tid; i < n; i += kFinishBS) {
    const orbx_keypoint kp = kps[i];
    orbx_keypoint kpu = kp;
    undistort_keypoint(A.cam, kpu);  // mvKeysUn[i]
    kun[i] = kpu;
    // imDepth.at<float>(v, u) with float v, u: truncation, at the DISTORTED keypoint (src/Frame.cc:799-806).
    // (-1, 0) truncates to 0 like the reference's; anything else outside the image (NaN too) is
    // counted and never read
    float d = -1.0f;
    if (kp.x > -1.0f && kp.x < (float)A.w && kp.y > -1.0f && kp.y < (float)A.h) {
      const int row = (int)kp.y, col = (int)kp.x;
      const uint8_t* r = img + (long long)row * A.depth_pitch;
      if (A.depth_type == ORBX_DEPTH_U16) {
        d = (float)((const uint16_t*)r)[col] * A.factor;  // convertTo(CV_32F, mDepthMapFactor)
      } else {
        const float raw = ((const float*)r)[col];
        d = A.scale ? raw * A.factor : raw;
      }
    } else {
      oob++;
    }
    if (d > 0) {  // src/Frame.cc:808-814
      dep[i] = d;
      uR[i] = kpu.x - A.bf / d;
      pos++;
    } else {
      dep[i] = -1.0f;
      uR[i] = -1.0f;
    }
  }
  pos = wave_sum(pos);
  oob = wave_sum(oob);
  if ((tid & 63) == 0) {
    if (pos) atomicAdd(&s_sum[0], pos);
    if (oob) atomicAdd(&s_sum[1], oob);
  }
  __syncthreads();
  if (tid == 0) {
    A.nmatches[f] = s_sum[0];
    A.n_oob[f] = s_sum[1];
  }
}

}  // namespace

hipError_t launch_cvt_gray(const CvtGrayArgs& A, int channels, hipStream_t st) {
  if (A.n <= 0 || A.w <= 0 || A.h <= 0) return hipSuccess;
  const int items = (A.w + 3) / 4 + 1;  // head + dwords (a row off the boundary splits one into head and tail)
  const dim3 grid((items + kGrayBX - 1) / kGrayBX, (A.h + kGrayBY - 1) / kGrayBY, A.n), block(kGrayBX, kGrayBY);
  if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
  if (channels == 3)
    hipLaunchKernelGGL(k_cvt_gray<3>, grid, block, 0, st, A);
  else
    hipLaunchKernelGGL(k_cvt_gray<4>, grid, block, 0, st, A);
  return hipGetLastError();
}

hipError_t launch_rgbd_finish(const RgbdFinishArgs& A, int n_frames, hipStream_t st) {
  if (n_frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rgbd_finish, dim3(n_frames), dim3(kFinishBS), 0, st, A);
  return hipGetLastError();
}

}  // namespace orbx

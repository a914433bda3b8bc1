// orbx_rgbd.h -- argument blocks and launchers of the RGB-D front end (rgbd.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbx.h"

namespace orbx {

// OpenCV 3.2 RGB2Gray<uchar>: Y = (R * R2Y + G * G2Y + B * B2Y + (1 << (yuv_shift - 1))) >> yuv_shift
constexpr int kR2Y = 4899, kG2Y = 9617, kB2Y = 1868, kYuvShift = 14;

// k_cvt_gray: n images of w x h pixels with `channels` (3 or 4) bytes each; row y of image i at
// src + i * src_image_pitch + y * src_pitch, its grey row at dst + i * dst_image_pitch + y * dst_pitch.
struct CvtGrayArgs {
  const uint8_t* src;
  uint8_t* dst;
  long long src_pitch, src_image_pitch, dst_pitch, dst_image_pitch;
  int w, h, n;
  int c0, c2;  // weights of byte 0 and byte 2 of a pixel (R2Y or B2Y, by the byte order)
};
hipError_t launch_cvt_gray(const CvtGrayArgs& A, int channels, hipStream_t st);

// k_rgbd_finish: frame f's keypoints at kps + f * k_stride (counts[f * n_stride] of them, at most
// max_k), its depth image at depth + f * depth_image_pitch.  Outputs per frame at stride out_stride.
struct RgbdFinishArgs {
  const orbx_keypoint* kps;
  const int32_t* counts;
  long long k_stride, n_stride;
  int max_k;
  orbx_camera cam;
  const uint8_t* depth;
  long long depth_pitch, depth_image_pitch;  // bytes
  int depth_type;                            // ORBX_DEPTH_U16 / ORBX_DEPTH_F32
  int scale;                                 // f32 source: multiply by factor (else the bits pass through)
  float factor, bf;
  int w, h;
  orbx_keypoint* kps_un;
  float* uR;
  float* dep;
  long long out_stride;
  int32_t* nmatches;  // [n_frames]: keypoints with d > 0
  int32_t* n_oob;     // [n_frames]: keypoints whose depth index fell outside the image
};
hipError_t launch_rgbd_finish(const RgbdFinishArgs& A, int n_frames, hipStream_t st);

}  // namespace orbx

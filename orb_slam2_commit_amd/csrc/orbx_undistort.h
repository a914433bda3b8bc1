// orbx_undistort.h -- cv::undistortPoints with P = K for one keypoint (OpenCV 3.2 cvUndistortPoints),
// the device function behind k_undistort (mapping.hip) and k_rgbd_finish (rgbd.hip).
//
// All FP64 in cvUndistortPoints' operation order (-ffp-contract=off; AMDGPU f64 division is
// correctly rounded), so the result equals the oracle bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbx.h"

namespace orbx {

// what the host forms require of a camera before a kernel divides by its focal lengths
inline bool camera_ok(const orbx_camera& c) { return c.n_dist >= 4 && c.n_dist <= 5 && c.K[0] != 0.0f && c.K[4] != 0.0f; }

// Frame::UndistortKeyPoints for one keypoint (src/Frame.cc:471-506): kp.pt replaced, everything
// else kept; mDistCoef.at<float>(0)==0.0 leaves kp as it is (:474-478).
__device__ __forceinline__ void undistort_keypoint(const orbx_camera& cam, orbx_keypoint& kp) {
  if (cam.dist[0] == 0.0f) return;
  double kc[5] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 5; j++)
    if (j < cam.n_dist) kc[j] = cam.dist[j];
  double A[9];
#pragma unroll
  for (int j = 0; j < 9; j++) A[j] = cam.K[j];
  const double ifx = 1. / A[0], ify = 1. / A[4], cx = A[2], cy = A[5];
  double x = kp.x, y = kp.y;
  const double x0 = x = (x - cx) * ifx;
  const double y0 = y = (y - cy) * ify;
#pragma unroll
  for (int it = 0; it < 5; it++) {  // cvUndistortPoints: iters = 5 with distortion
    const double r2 = x * x + y * y;
    const double icdist = 1 / (1 + ((kc[4] * r2 + kc[1]) * r2 + kc[0]) * r2);
    const double deltaX = 2 * kc[2] * x * y + kc[3] * (r2 + 2 * x * x);
    const double deltaY = kc[2] * (r2 + 2 * y * y) + 2 * kc[3] * x * y;
    x = (x0 - deltaX) * icdist;
    y = (y0 - deltaY) * icdist;
  }
  const double xx = A[0] * x + A[1] * y + A[2];
  const double yy = A[3] * x + A[4] * y + A[5];
  const double ww = 1. / (A[6] * x + A[7] * y + A[8]);
  kp.x = (float)(xx * ww);
  kp.y = (float)(yy * ww);
}

}  // namespace orbx

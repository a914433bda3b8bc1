// orbx_match.h -- the tail every ORBmatcher search shares: the rotation histogram's bin and
// ComputeThreeMaxima.  The searches keep their own histogram filling and their own filtering loops.
#pragma once
#include <hip/hip_runtime.h>

namespace orbx {

// the rotation histogram's bin of a match (src/ORBmatcher.cc: rot = angle1 - angle2, + 360 when
// negative, round(rot * factor) with factor = 1.0f / HISTO_LENGTH, bin 30 is bin 0)
__host__ __device__ __forceinline__ int rot_bin(float a, float b) {
  float rot = a - b;
  if (rot < 0.0) rot += 360.0f;
  int bin = (int)__builtin_roundf(rot * (1.0f / 30));
  if (bin == 30) bin = 0;
  return bin;
}

// ComputeThreeMaxima, src/ORBmatcher.cc:1797-1839, of the 30 bins' sizes: the three largest, the
// first bin winning a tie (the comparisons are strict); the second and third are dropped (-1) when
// below 0.1f * the largest
__host__ __device__ __forceinline__ void three_maxima(const int* hist30, int* sel3) {
  int m1 = 0, m2 = 0, m3 = 0, i1 = -1, i2 = -1, i3 = -1;
  for (int b = 0; b < 30; b++) {
    const int s = hist30[b];
    if (s > m1) {
      m3 = m2; m2 = m1; m1 = s;
      i3 = i2; i2 = i1; i1 = b;
    } else if (s > m2) {
      m3 = m2; m2 = s;
      i3 = i2; i2 = b;
    } else if (s > m3) {
      m3 = s;
      i3 = b;
    }
  }
  if (m2 < 0.1f * (float)m1) {
    i2 = -1;
    i3 = -1;
  } else if (m3 < 0.1f * (float)m1) {
    i3 = -1;
  }
  sel3[0] = i1;
  sel3[1] = i2;
  sel3[2] = i3;
}

}  // namespace orbx

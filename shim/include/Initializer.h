// Initializer.h -- drop-in ORB_SLAM2::Initializer over liborbx.so (include/Initializer.h:36-45): the
// constructor copies the reference frame's mK and mvKeysUn (src/Initializer.cc:40-53); Initialize
// builds mvMatches12 from vMatches12, draws the 200 eight-point sets, and runs FindHomography /
// FindFundamental, the model choice and ReconstructH / ReconstructF on the MI355X (:58-1345),
// bit-exact with the reference's arithmetic.  Tracking::MonocularInitialization creates it as
// Initializer(mCurrentFrame, 1.0, 200) and feeds it ORBmatcher::SearchForInitialization's matches
// (src/Tracking.cc:683-730).
//
// Random numbers: Initialize calls DUtils::Random::SeedRandOnce(0) (:106), which seeds the process
// rand() on the first call only, then draws 8 values per iteration from it.  The shim does the
// same on its one shared glibc-rand() stream (the PnPsolver's and Sim3Solver's).
#pragma once
#include <vector>

#include "Objects.h"
#include "opencv_min.hpp"
#include "orbx.h"

namespace ORB_SLAM2 {

class Initializer {
 public:
  // Fix the reference frame
  Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200);
  ~Initializer();
  Initializer(const Initializer&) = delete;
  Initializer& operator=(const Initializer&) = delete;

  // Computes in parallel a fundamental matrix and a homography, selects a model and tries to
  // recover the motion and the structure.  R21 (3x3 CV_32F) and t21 (3x1 CV_32F) are released
  // (empty) on false, as the reference leaves them; vP3D / vbTriangulated are then untouched.
  // Fewer than 8 matches throw std::runtime_error (the reference underflows size() - 1 there).
  bool Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
                  std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated);

  orbx_initializer_result mResult{};  // the stage results of the last call (not in the reference)

 private:
  std::vector<cv::KeyPoint> mvKeys1;  // Keypoints from Reference Frame (Frame 1)
  cv::Mat mK;                         // Calibration
  float mSigma = 1.f;
  int mMaxIterations = 200;
  orbx_initializer* mpGpu = nullptr;
};

}  // namespace ORB_SLAM2

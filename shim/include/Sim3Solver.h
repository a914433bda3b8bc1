// Sim3Solver.h -- drop-in ORB_SLAM2::Sim3Solver over liborbx.so (include/Sim3Solver.h:36-50): the
// constructor gathers the 3D-3D correspondences of two KeyFrames' MapPoint matches exactly as
// src/Sim3Solver.cc:37-125 does (vpMatched12[i1] set, vpKeyFrameMP1[i1] set, neither MapPoint bad,
// both GetIndexInKeyFrame >= 0; camera-frame points Rcw*X + tcw, mvLevelSigma2 of the two keypoints'
// octaves), SetRansacParameters derives mRansacMaxIts and resets mnIterations (:127-151), and
// iterate()/find() run the Horn RANSAC with CheckInliers on the MI355X (:153-422), bit-exact with
// the reference's arithmetic.
//
// Random numbers: DUtils::Random::RandomInt draws from the process rand(); every Sim3Solver draws
// from the shim's one shared glibc-rand() stream (the PnPsolver's: PnPsolver::SeedRandom restarts
// it), so LoopClosing::ComputeSim3's round-robin over candidate solvers (src/LoopClosing.cc:372-402)
// consumes the stream exactly as the reference does.
#pragma once
#include <vector>

#include "Objects.h"
#include "opencv_min.hpp"
#include "orbx.h"

namespace ORB_SLAM2 {

class Sim3Solver {
 public:
  Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true);
  ~Sim3Solver();
  Sim3Solver(const Sim3Solver&) = delete;
  Sim3Solver& operator=(const Sim3Solver&) = delete;

  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);

  cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers);
  // Returns T12 (4x4 CV_32F) or an empty Mat; vbInliers has vpMatched12.size() entries.
  cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

  cv::Mat GetEstimatedRotation();     // 3x3 CV_32F (zeros before the first iteration)
  cv::Mat GetEstimatedTranslation();  // 3x1 CV_32F
  float GetEstimatedScale();

 private:
  void ensure_solver();
  int mN1 = 0;
  std::vector<size_t> mvnIndices1;
  std::vector<float> mvX3Dc1, mvX3Dc2, mvSigma2_1, mvSigma2_2;  // x,y,z / sigma^2 per correspondence
  float mK1[4] = {0, 0, 0, 0}, mK2[4] = {0, 0, 0, 0};         // fx, fy, cx, cy
  bool mbFixScale = true;
  orbx_sim3_params mParams{0.99, 6, 300};
  int mRansacMaxIts = 0;
  orbx_sim3* mpGpu = nullptr;
};

}  // namespace ORB_SLAM2

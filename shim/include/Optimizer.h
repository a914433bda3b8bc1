// Optimizer.h -- Optimizer::LocalBundleAdjustment (include/Optimizer.h:61, src/Optimizer.cc:530-885)
// over liborbx.so.  Two forms:
//   * the reference signature LocalBundleAdjustment(KeyFrame*, bool*, Map*): the shim gathers the
//     local window from the object graph exactly as src/Optimizer.cc:532-745 does (covisible
//     KeyFrames, their MapPoints, the fixed cameras that observe them, one edge per observation in
//     GetObservations() order), runs it on the MI355X, and applies the result as :817-884 does
//     (EraseMapPointMatch / EraseObservation under Map::mMutexMapUpdate, SetPose, SetWorldPos,
//     UpdateNormalAndDepth);
//   * the same on an explicit problem (the caller gathers and applies).
// g2o semantics (BlockSolver_6_3, LinearSolverEigen, Levenberg, Huber kernels, optimize(5),
// outlier levels, optimize(10)) run in FP64 on the MI355X.
#pragma once
#include <array>
#include <map>
#include <set>
#include <vector>

#include "g2o_sim3_min.h"
#include "opencv_min.hpp"

namespace ORB_SLAM2 {

class MapPoint;

struct LocalBAProblem {
  struct Camera {
    cv::Mat Tcw;                    // 4x4 CV_32F, KeyFrame::GetPose()
    bool fixed = false;             // mnId == 0, or a member of lFixedCameras
    float fx = 0, fy = 0, cx = 0, cy = 0, bf = 0;
  };
  struct Observation {              // one edge per (KeyFrame, MapPoint) observation, in the reference's order
    int point = 0, camera = 0;
    float u = 0, v = 0;             // mvKeysUn[idx].pt
    float ur = -1;                  // mvuRight[idx]; < 0: monocular EdgeSE3ProjectXYZ
    float invSigma2 = 1;            // mvInvLevelSigma2[octave]
  };
  std::vector<Camera> cameras;
  std::vector<cv::Mat> points;      // 3x1 CV_32F, MapPoint::GetWorldPos()
  std::vector<Observation> observations;
};

struct LocalBAResult {
  std::vector<cv::Mat> Tcw;         // 4x4 CV_32F per camera (Converter::toCvMat of the optimised SE3Quat)
  std::vector<cv::Mat> points;      // 3x1 CV_32F per point
  std::vector<bool> erase;          // per observation: vToErase (:817-847)
  int iterations[2] = {0, 0};       // LM iterations of optimize(5) and optimize(10)
  int trials = 0;
  bool ran = false;                 // false: stopped before optimize(5), outputs are the inputs (:749-751)
};

class KeyFrame;
class Map;
class Frame;

class KeyFrame;
class Map;

// include/LoopClosing.h:48-50: the typedef OptimizeEssentialGraph's signature names (the reference adds an
// Eigen aligned allocator, which the Sim3 slice of g2o_sim3_min.h does not need)
class LoopClosing {
 public:
  typedef std::map<KeyFrame*, g2o::Sim3, std::less<KeyFrame*>> KeyFrameAndPose;
};

class Optimizer {
 public:
  // include/Optimizer.h:71, src/Optimizer.cc:287-528: the pose of pFrame from its MapPoint matches
  // (four rounds of optimize(10) with outlier levels, on the MI355X).  Sets pFrame->mvbOutlier and,
  // with >= 3 correspondences, pFrame->SetPose; returns the inlier count (0 below 3 matches).
  int static PoseOptimization(Frame* pFrame);
  // include/Optimizer.h:61.  pbStopFlag: the reference's bool* (NULL allowed), polled before the
  // run and between LM trials.  Runs on device gOrbxDevice.  Throws std::runtime_error on a library
  // error (the object graph is then left as it was).
  void static LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap);
  // The explicit-problem form.  Throws std::runtime_error on a library error.
  void static LocalBundleAdjustment(const LocalBAProblem& problem, bool* pbStopFlag, LocalBAResult& result,
                                    int device = 0);

  // include/Optimizer.h:48-54, src/Optimizer.cc:41-284 (called at src/Tracking.cc CreateInitialMapMonocular
  // and src/LoopClosing.cc RunGlobalBundleAdjustment): one optimize(nIterations) over every keyframe and
  // map point given, on the MI355X.  Gathers as :75-218 does -- keyframes that are not bad (fixed for
  // mnId == 0), points that are not bad, the observations whose keyframe is not bad and has mnId <=
  // maxKFid -- walking keyframes, points and each point's observations in ASCENDING mnId (the reference
  // walks its containers in pointer order; the order changes summation order only).  Writes back per
  // :228-282: nLoopKF == 0 SetPose / SetWorldPos / UpdateNormalAndDepth, otherwise mTcwGBA / mPosGBA /
  // mnBAGlobalForKF; a point that ended with no edge (vbNotIncludedMP) is left alone.  Up to 512 free
  // keyframes; throws std::runtime_error on a library error (the object graph is then left as it was).
  void static BundleAdjustment(const std::vector<KeyFrame*>& vpKF, const std::vector<MapPoint*>& vpMP,
                               int nIterations = 5, bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0,
                               const bool bRobust = true);
  void static GlobalBundleAdjustemnt(Map* pMap, int nIterations = 5, bool* pbStopFlag = NULL,
                                     const unsigned long nLoopKF = 0, const bool bRobust = true);

  // include/Optimizer.h, src/Optimizer.cc:1220-1456 (called at src/LoopClosing.cc:425-444): refines
  // g2oS12 over the matches of vpMatches1 (per keypoint of pKF1, the MapPoint of pKF2 or NULL) on the
  // MI355X.  Gathers as :1267-1384 does, nulls the outliers in vpMatches1, writes g2oS12 only when
  // the reference does (not on the early return below 10 survivors) and returns the inlier count.
  int static OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12,
                          const float th2, const bool bFixScale);

  // include/Optimizer.h, src/Optimizer.cc:888-1218 (called at src/LoopClosing.cc:785): the pose graph over
  // every keyframe of pMap on the MI355X.  Vertices and edges as :929-1138 selects them (keyframes and the
  // pointer-ordered containers walked in ascending mnId; a bad keyframe gets no vertex and keeps its
  // pose), then under pMap->mMutexMapUpdate SetPose of every vertex's keyframe and SetWorldPos +
  // UpdateNormalAndDepth of every point that is not bad, as :1144-1217 does.
  void static OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF,
                                     const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                     const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                                     const std::map<KeyFrame*, std::set<KeyFrame*>>& LoopConnections,
                                     const bool& bFixScale);

  // test hook: called with the window the graph form gathered, before it runs (NULL: none)
  static void (*mpfnGatheredHook)(const LocalBAProblem& problem, const std::vector<KeyFrame*>& cameras);
};

}  // namespace ORB_SLAM2

// LocalMapping.h -- ORB_SLAM2::LocalMapping's CreateNewMapPoints over liborbx.so
// (include/LocalMapping.h:39-134, src/LocalMapping.cc:281-558).  The constructor, InsertKeyFrame and
// CheckNewKeyFrames are the reference's; CreateNewMapPoints() takes
// mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn), gathers the keyframes once, makes ONE
// orbx_create_new_map_points call (the neighbour chain runs on the MI355X), and then, in the returned
// order (neighbour, ascending idx1), does what :539-553 does per accepted pair: new MapPoint, both
// AddObservation, both AddMapPoint, ComputeDistinctiveDescriptors, UpdateNormalAndDepth,
// Map::AddMapPoint, push to mlpRecentAddedMapPoints.
//
// KeyFrameCulling() (:784-871) runs over the Map's device-resident covisibility table.
//
// CheckNewKeyFrames() between neighbours (:320) is the handle's device-readable flag: InsertKeyFrame
// raises it, CreateNewMapPoints sets it from mlNewKeyFrames on entry.  The first neighbour always runs.
// The thread loop (Run, ProcessNewKeyFrame, MapPointCulling, SearchInNeighbors) stays
// with the caller; the reference's protected members the caller of this step touches are public here.
#pragma once
#include <list>
#include <mutex>

#include "Objects.h"
#include "orbx.h"

namespace ORB_SLAM2 {

class LocalMapping {
 public:
  LocalMapping(Map* pMap, const float bMonocular);  // include/LocalMapping.h:44
  ~LocalMapping();
  LocalMapping(const LocalMapping&) = delete;
  LocalMapping& operator=(const LocalMapping&) = delete;

  void InsertKeyFrame(KeyFrame* pKF);  // src/LocalMapping.cc:141-146
  bool CheckNewKeyFrames();            // :149-153
  void CreateNewMapPoints();           // :281-558
  // :784-871 over the Map's covisibility table: ONE orbx_covis_cull call judges
  // mpCurrentKeyFrame->GetVectorCovisibleKeyFrames() in order on the MI355X (verdicts, cascades and the points
  // that go bad included), then the object-graph half of KeyFrame::SetBadFlag (src/KeyFrame.cc:581-677) is
  // applied here per verdict.  The table must hold the current rows (Map::UploadCovisibilityRow).
  void KeyFrameCulling();

  Map* mpMap;
  bool mbMonocular;
  bool mbAbortBA = false;
  KeyFrame* mpCurrentKeyFrame = nullptr;
  std::list<KeyFrame*> mlNewKeyFrames;
  std::list<MapPoint*> mlpRecentAddedMapPoints;
  std::mutex mMutexNewKFs;
  int mnNeighboursDone = 0;  // loop bodies entered by the last call (not in the reference)

 private:
  orbx_new_points* mpGpu = nullptr;
  volatile int* mpFlag = nullptr;
};

}  // namespace ORB_SLAM2

// Objects.h -- the fields and methods of ORB-SLAM2's Frame / KeyFrame / MapPoint / Map (and DBoW2's
// FeatureVector) that the hot-path members read or mutate, with the reference's names and
// signatures.  Inside ORB-SLAM2 these are the real classes (include/Frame.h, include/KeyFrame.h,
// include/MapPoint.h, include/Map.h) and shim.cc compiles against them unchanged; here they are
// minimal stand-ins the shim's tests build object graphs from.  Bodies restate the reference's
// (src/KeyFrame.cc, src/MapPoint.cc, src/Frame.cc) for exactly the members the shim's hot-path
// bodies use: LocalBundleAdjustment's gather and write-back, SearchByProjection x3, Fuse's
// Replace/AddObservation, SearchForTriangulation, PoseOptimization, ComputeDistinctiveDescriptors
// and ComputeBoW.
#pragma once
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "opencv_min.hpp"

struct orbx_covis;  // include/orbx.h: the device-resident covisibility table a Map owns

namespace DBoW2 {
typedef unsigned int NodeId;
typedef unsigned int WordId;
typedef double WordValue;
// Thirdparty/DBoW2/DBoW2/FeatureVector.h: node id -> indices of the features under it (ascending ids)
class FeatureVector : public std::map<NodeId, std::vector<unsigned int>> {};
// Thirdparty/DBoW2/DBoW2/BowVector.h: word id -> weight (ascending ids)
class BowVector : public std::map<WordId, WordValue> {};
}  // namespace DBoW2

namespace ORB_SLAM2 {

class ORBextractor;
class ORBVocabulary;
class KeyFrame;
class Map;

class MapPoint {
 public:
  MapPoint() = default;
  MapPoint(const cv::Mat& Pos, KeyFrame* pRefKF, Map* pMap) : mpRefKF(pRefKF), mpMap(pMap) { SetWorldPos(Pos); }

  void SetWorldPos(const cv::Mat& Pos) {  // include/MapPoint.h:45
    std::unique_lock<std::mutex> lock(mMutexPos);
    Pos.copyTo(mWorldPos);
  }
  cv::Mat GetWorldPos() {  // include/MapPoint.h:46
    std::unique_lock<std::mutex> lock(mMutexPos);
    return mWorldPos.clone();
  }
  cv::Mat GetNormal() {
    std::unique_lock<std::mutex> lock(mMutexPos);
    return mNormalVector.clone();
  }
  std::map<KeyFrame*, size_t> GetObservations() {  // include/MapPoint.h:52
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    return mObservations;
  }
  int Observations() {
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    return nObs;
  }
  void AddObservation(KeyFrame* pKF, size_t idx);  // src/MapPoint.cc AddObservation
  void EraseObservation(KeyFrame* pKF);            // src/MapPoint.cc EraseObservation
  int GetIndexInKeyFrame(KeyFrame* pKF) {          // include/MapPoint.h:66
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    auto it = mObservations.find(pKF);
    return it == mObservations.end() ? -1 : (int)it->second;
  }
  void SetBadFlag();                                // src/MapPoint.cc SetBadFlag
  bool isBad() {                                    // include/MapPoint.h: isBad()
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    return mbBad;
  }
  void UpdateNormalAndDepth();                      // src/MapPoint.cc UpdateNormalAndDepth
  float GetMinDistanceInvariance() {
    std::unique_lock<std::mutex> lock(mMutexPos);
    return 0.8f * mfMinDistance;
  }
  float GetMaxDistanceInvariance() {
    std::unique_lock<std::mutex> lock(mMutexPos);
    return 1.2f * mfMaxDistance;
  }
  cv::Mat GetDescriptor() {                         // src/MapPoint.cc:323-327
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    return mDescriptor.clone();
  }
  bool IsInKeyFrame(KeyFrame* pKF) {                // src/MapPoint.cc IsInKeyFrame
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    return mObservations.count(pKF) > 0;
  }
  void IncreaseVisible(int n = 1) {
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    mnVisible += n;
  }
  void IncreaseFound(int n = 1) {
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    mnFound += n;
  }
  void Replace(MapPoint* pMP);                      // src/MapPoint.cc:179-221
  KeyFrame* GetReferenceKeyFrame() {                // src/MapPoint.cc:92-96
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    return mpRefKF;
  }
  // MapPoint::ComputeDistinctiveDescriptors (include/MapPoint.h:85, src/MapPoint.cc:249-320): the
  // observed descriptor with the least median Hamming distance to the others, on the MI355X
  // (defined in shim.cc over orbx_distinctive_descriptors)
  void ComputeDistinctiveDescriptors();

  long unsigned int mnId = 0;
  long unsigned int mnBALocalForKF = 0, mnFuseCandidateForKF = 0;
  // written by LoopClosing::CorrectLoop, read by OptimizeEssentialGraph (include/MapPoint.h:130-133)
  long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
  // written by Optimizer::BundleAdjustment with nLoopKF != 0 (include/MapPoint.h:135-136): the global
  // bundle adjustment's position, applied later by LoopClosing::RunGlobalBundleAdjustment
  cv::Mat mPosGBA;
  long unsigned int mnBAGlobalForKF = 0;
  int nObs = 0;
  int mnVisible = 1, mnFound = 1;
  bool mbBad = false;
  MapPoint* mpReplaced = nullptr;
  cv::Mat mWorldPos, mNormalVector;
  cv::Mat mDescriptor;  // 1 x 32 CV_8U (the best descriptor)
  float mfMinDistance = 0.f, mfMaxDistance = 0.f;
  // Tracking::SearchLocalPoints' frustum test results read by SearchByProjection(Frame&, vector<MapPoint*>)
  bool mbTrackInView = false;
  float mTrackProjX = 0.f, mTrackProjY = 0.f, mTrackProjXR = 0.f, mTrackViewCos = 0.f;
  int mnTrackScaleLevel = 0;
  std::map<KeyFrame*, size_t> mObservations;
  KeyFrame* mpRefKF = nullptr;
  Map* mpMap = nullptr;
  std::mutex mMutexPos, mMutexFeatures;
};

class KeyFrame {
 public:
  void SetPose(const cv::Mat& Tcw_);  // src/KeyFrame.cc SetPose (Tcw, Ow)
  cv::Mat GetPose() {                  // include/KeyFrame.h:50
    std::unique_lock<std::mutex> lock(mMutexPose);
    return Tcw.clone();
  }
  cv::Mat GetCameraCenter() {          // include/KeyFrame.h:52
    std::unique_lock<std::mutex> lock(mMutexPose);
    return Ow.clone();
  }
  // covisibility graph order (weights descending), src/KeyFrame.cc GetVectorCovisibleKeyFrames
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() {
    std::unique_lock<std::mutex> lock(mMutexConnections);
    return mvpOrderedConnectedKeyFrames;
  }
  // src/KeyFrame.cc:224-232: the first N of the ordered list (all of it when shorter)
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
    std::unique_lock<std::mutex> lock(mMutexConnections);
    if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
    return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
  }
  // src/KeyFrame.cc:198-205: every connected keyframe (the keys of mConnectedKeyFrameWeights, which
  // the ordered list holds too)
  std::set<KeyFrame*> GetConnectedKeyFrames() {
    std::unique_lock<std::mutex> lock(mMutexConnections);
    return std::set<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.end());
  }
  void EraseMapPointMatch(const size_t& idx) {  // include/KeyFrame.h:103
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    mvpMapPoints[idx] = nullptr;
  }
  void EraseMapPointMatch(MapPoint* pMP) {      // include/KeyFrame.h:104
    const int idx = pMP->GetIndexInKeyFrame(this);
    if (idx >= 0) mvpMapPoints[idx] = nullptr;
  }
  std::vector<MapPoint*> GetMapPointMatches() {  // src/KeyFrame.cc
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    return mvpMapPoints;
  }
  std::set<MapPoint*> GetMapPoints();           // src/KeyFrame.cc GetMapPoints: the non-bad MapPoints
  MapPoint* GetMapPoint(const size_t& idx) {     // src/KeyFrame.cc GetMapPoint
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    return mvpMapPoints[idx];
  }
  void AddMapPoint(MapPoint* pMP, const size_t& idx) {  // src/KeyFrame.cc AddMapPoint
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    mvpMapPoints[idx] = pMP;
  }
  void ReplaceMapPointMatch(const size_t& idx, MapPoint* pMP) { mvpMapPoints[idx] = pMP; }
  cv::Mat GetRotation() {                        // Tcw.rowRange(0,3).colRange(0,3)
    std::unique_lock<std::mutex> lock(mMutexPose);
    cv::Mat R(3, 3, CV_32F);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) R.at<float>(r, c) = Tcw.at<float>(r, c);
    return R;
  }
  cv::Mat GetTranslation() {                     // Tcw.rowRange(0,3).col(3)
    std::unique_lock<std::mutex> lock(mMutexPose);
    cv::Mat t(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) t.at<float>(r, 0) = Tcw.at<float>(r, 3);
    return t;
  }
  bool IsInImage(const float& x, const float& y) const {  // src/KeyFrame.cc:749-752
    return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY);
  }
  void ComputeBoW();                             // src/KeyFrame.cc ComputeBoW (defined in shim.cc)
  bool isBad() { return mbBad; }
  // src/KeyFrame.cc:239-255: the ordered covisibles whose weight is at least w
  std::vector<KeyFrame*> GetCovisiblesByWeight(const int& w) {
    std::unique_lock<std::mutex> lock(mMutexConnections);
    if (mvpOrderedConnectedKeyFrames.empty()) return std::vector<KeyFrame*>();
    std::vector<int>::iterator it = std::upper_bound(mvOrderedWeights.begin(), mvOrderedWeights.end(), w, weightComp);
    if (it == mvOrderedWeights.end()) return std::vector<KeyFrame*>();
    const int n = (int)(it - mvOrderedWeights.begin());
    return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + n);
  }
  int GetWeight(KeyFrame* pKF) {                 // src/KeyFrame.cc:261-268
    std::unique_lock<std::mutex> lock(mMutexConnections);
    if (mConnectedKeyFrameWeights.count(pKF)) return mConnectedKeyFrameWeights[pKF];
    return 0;
  }
  KeyFrame* GetParent() {                        // src/KeyFrame.cc:520-524
    std::unique_lock<std::mutex> lockCon(mMutexConnections);
    return mpParent;
  }
  bool hasChild(KeyFrame* pKF) {                 // src/KeyFrame.cc:526-530
    std::unique_lock<std::mutex> lockCon(mMutexConnections);
    return mspChildrens.count(pKF) > 0;
  }
  std::set<KeyFrame*> GetLoopEdges() {           // src/KeyFrame.cc:539-543
    std::unique_lock<std::mutex> lockCon(mMutexConnections);
    return mspLoopEdges;
  }
  static bool weightComp(int a, int b) { return a > b; }  // include/KeyFrame.h:141-143

  // Covisibility graph and spanning tree (include/KeyFrame.h:66-134, src/KeyFrame.cc:147-192, 367-565, 686-700).
  // UpdateConnections takes steps 1-2 (KFcounter, the threshold, the order) from the Map's device-resident
  // table (orbx_covis_update_connections) and applies step 3 and the other keyframes' AddConnection here; the
  // table must hold the current rows (Map::UploadCovisibilityRow).  Throws without mpMap or without a device.
  void UpdateConnections();
  void AddConnection(KeyFrame* pKF, const int& weight) {  // src/KeyFrame.cc:147-162
    {
      std::unique_lock<std::mutex> lock(mMutexConnections);
      if (!mConnectedKeyFrameWeights.count(pKF))
        mConnectedKeyFrameWeights[pKF] = weight;
      else if (mConnectedKeyFrameWeights[pKF] != weight)
        mConnectedKeyFrameWeights[pKF] = weight;
      else
        return;
    }
    UpdateBestCovisibles();
  }
  void EraseConnection(KeyFrame* pKF) {  // src/KeyFrame.cc:686-700
    bool bUpdate = false;
    {
      std::unique_lock<std::mutex> lock(mMutexConnections);
      if (mConnectedKeyFrameWeights.count(pKF)) {
        mConnectedKeyFrameWeights.erase(pKF);
        bUpdate = true;
      }
    }
    if (bUpdate) UpdateBestCovisibles();
  }
  void UpdateBestCovisibles();  // src/KeyFrame.cc:169-192 (pairs ordered by weight, then by mnId for pointer order)
  void AddChild(KeyFrame* pKF) {  // src/KeyFrame.cc:495-499
    std::unique_lock<std::mutex> lockCon(mMutexConnections);
    mspChildrens.insert(pKF);
  }
  void EraseChild(KeyFrame* pKF) {  // src/KeyFrame.cc:501-505
    std::unique_lock<std::mutex> lockCon(mMutexConnections);
    mspChildrens.erase(pKF);
  }
  void ChangeParent(KeyFrame* pKF) {  // src/KeyFrame.cc:507-512
    {
      std::unique_lock<std::mutex> lockCon(mMutexConnections);
      mpParent = pKF;
    }
    pKF->AddChild(this);
  }
  std::set<KeyFrame*> GetChilds() {  // src/KeyFrame.cc:514-518
    std::unique_lock<std::mutex> lockCon(mMutexConnections);
    return mspChildrens;
  }
  void SetNotErase() {  // src/KeyFrame.cc:545-549
    std::unique_lock<std::mutex> lock(mMutexConnections);
    mbNotErase = true;
  }
  // src/KeyFrame.cc:567-678.  SetBadFlag() also takes the keyframe's row out of the Map's table (when the Map has
  // one and the row is there) and reports the points that went bad to it; SetBadFlagHost() is the object-graph
  // half alone, for LocalMapping::KeyFrameCulling, whose device call has done the table's half already.  Returns
  // false when nothing happened (mnId 0, or mbNotErase: mbToBeErased is set).
  void SetBadFlag();
  bool SetBadFlagHost();

  long unsigned int mnId = 0;
  long unsigned int mnBALocalForKF = 0, mnBAFixedForKF = 0;
  // written by Optimizer::BundleAdjustment with nLoopKF != 0 (include/KeyFrame.h:197-199)
  cv::Mat mTcwGBA;
  long unsigned int mnBAGlobalForKF = 0;
  // written by KeyFrameDatabase (include/KeyFrame.h:181-194); the two scores are uninitialised in the
  // reference and start at 0 here, as on the device
  long unsigned int mnLoopQuery = 0;
  int mnLoopWords = 0;
  float mLoopScore = 0.f;
  long unsigned int mnRelocQuery = 0;
  int mnRelocWords = 0;
  float mRelocScore = 0.f;
  float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0, mbf = 0, mb = 0, mThDepth = 0;
  int N = 0;
  std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
  std::vector<float> mvuRight, mvDepth;  // negative: monocular
  cv::Mat mDescriptors;                  // N x 32 CV_8U
  DBoW2::BowVector mBowVec;
  DBoW2::FeatureVector mFeatVec;
  ORBVocabulary* mpORBvocabulary = nullptr;
  // the Frame's image bounds and grid, copied at KeyFrame creation (include/KeyFrame.h: const int mnMinX..)
  int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
  float mfGridElementWidthInv = 0.f, mfGridElementHeightInv = 0.f;
  int mnScaleLevels = 8;
  float mfScaleFactor = 1.2f, mfLogScaleFactor = 0.f;
  std::vector<float> mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
  // the covisibility weights beside the ordered list, the spanning tree and the loop edges
  // (include/KeyFrame.h:214-224)
  std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
  std::vector<int> mvOrderedWeights;
  KeyFrame* mpParent = nullptr;
  std::set<KeyFrame*> mspChildrens, mspLoopEdges;
  bool mbFirstConnection = true;                    // include/KeyFrame.h:280
  bool mbNotErase = false, mbToBeErased = false;   // include/KeyFrame.h:290-291
  bool mbBad = false;
  Map* mpMap = nullptr;                             // include/KeyFrame.h:296
  cv::Mat Tcw, Ow;
  std::mutex mMutexPose, mMutexConnections, mMutexFeatures;
};

class Map {
 public:
  Map() = default;
  ~Map();  // (shim.cc: destroys the covisibility table)
  Map(const Map&) = delete;
  Map& operator=(const Map&) = delete;
  void AddKeyFrame(KeyFrame* pKF) {    // src/Map.cc:39-45
    std::unique_lock<std::mutex> lock(mMutexMap);
    mspKeyFrames.insert(pKF);
    if (pKF->mnId > mnMaxKFid) mnMaxKFid = pKF->mnId;
  }
  void EraseKeyFrame(KeyFrame* pKF) {  // src/Map.cc:62-68
    std::unique_lock<std::mutex> lock(mMutexMap);
    mspKeyFrames.erase(pKF);
  }
  // The device-resident covisibility table (orbx_covis, include/orbx.h), created on first use; throws
  // std::runtime_error without a device.  Not in the reference: it is what KeyFrame::UpdateConnections and
  // LocalMapping::KeyFrameCulling scan instead of walking mObservations.
  orbx_covis* Covisibility();
  // Uploads pKF's whole row from mvpMapPoints / mvKeysUn[i].octave / mvuRight / mvDepth / mThDepth (a bad
  // MapPoint goes up as "none"): after ProcessNewKeyFrame, Fuse / Replace, AddMapPoint / EraseMapPointMatch.
  void UploadCovisibilityRow(KeyFrame* pKF);
  // MapPoint::SetBadFlag / Replace seen from the table
  void CovisibilityPointsBad(const std::vector<MapPoint*>& vpMP);
  // the objects behind the table's ids (nullptr when the table has never seen the id)
  KeyFrame* CovisibilityKeyFrame(long unsigned int id) {
    auto it = mCovisKFs.find(id);
    return it == mCovisKFs.end() ? nullptr : it->second;
  }
  MapPoint* CovisibilityMapPoint(long unsigned int id) {
    auto it = mCovisMPs.find(id);
    return it == mCovisMPs.end() ? nullptr : it->second;
  }
  std::map<long unsigned int, KeyFrame*> mCovisKFs;  // the rows the table holds
  std::map<long unsigned int, MapPoint*> mCovisMPs;  // every point uploaded in a row
  void AddMapPoint(MapPoint* pMP) {    // src/Map.cc:48-52
    std::unique_lock<std::mutex> lock(mMutexMap);
    mspMapPoints.insert(pMP);
  }
  void EraseMapPoint(MapPoint* pMP) {  // src/Map.cc EraseMapPoint
    std::unique_lock<std::mutex> lock(mMutexMap);
    mspMapPoints.erase(pMP);
  }
  std::vector<KeyFrame*> GetAllKeyFrames() {  // src/Map.cc:82-86
    std::unique_lock<std::mutex> lock(mMutexMap);
    return std::vector<KeyFrame*>(mspKeyFrames.begin(), mspKeyFrames.end());
  }
  std::vector<MapPoint*> GetAllMapPoints() {  // src/Map.cc:88-92
    std::unique_lock<std::mutex> lock(mMutexMap);
    return std::vector<MapPoint*>(mspMapPoints.begin(), mspMapPoints.end());
  }
  long unsigned int GetMaxKFid() {            // src/Map.cc:112-116
    std::unique_lock<std::mutex> lock(mMutexMap);
    return mnMaxKFid;
  }
  std::set<MapPoint*> mspMapPoints;
  std::set<KeyFrame*> mspKeyFrames;
  long unsigned int mnMaxKFid = 0;
  std::mutex mMutexMapUpdate;  // include/Map.h:65
  std::mutex mMutexMap;

 private:
  orbx_covis* mpCovis = nullptr;
};

// ---- the reference bodies (src/MapPoint.cc, src/KeyFrame.cc), restated for the stand-ins
inline void MapPoint::AddObservation(KeyFrame* pKF, size_t idx) {
  std::unique_lock<std::mutex> lock(mMutexFeatures);
  if (mObservations.count(pKF)) return;
  mObservations[pKF] = idx;
  if (pKF->mvuRight[idx] >= 0)
    nObs += 2;
  else
    nObs++;
}

inline void MapPoint::EraseObservation(KeyFrame* pKF) {
  bool bBad = false;
  {
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    if (mObservations.count(pKF)) {
      const int idx = (int)mObservations[pKF];
      if (pKF->mvuRight[idx] >= 0)
        nObs -= 2;
      else
        nObs--;
      mObservations.erase(pKF);
      if (mpRefKF == pKF) mpRefKF = mObservations.empty() ? nullptr : mObservations.begin()->first;
      if (nObs <= 2) bBad = true;
    }
  }
  if (bBad) SetBadFlag();
}

inline void MapPoint::SetBadFlag() {
  std::map<KeyFrame*, size_t> obs;
  {
    std::unique_lock<std::mutex> lock1(mMutexFeatures);
    std::unique_lock<std::mutex> lock2(mMutexPos);
    mbBad = true;
    obs = mObservations;
    mObservations.clear();
  }
  for (auto& o : obs) o.first->EraseMapPointMatch(o.second);
  if (mpMap) mpMap->EraseMapPoint(this);
}

inline void MapPoint::UpdateNormalAndDepth() {
  std::map<KeyFrame*, size_t> observations;
  KeyFrame* pRefKF;
  cv::Mat Pos;
  {
    std::unique_lock<std::mutex> lock1(mMutexFeatures);
    std::unique_lock<std::mutex> lock2(mMutexPos);
    if (mbBad) return;
    observations = mObservations;
    pRefKF = mpRefKF;
    Pos = mWorldPos.clone();
  }
  if (observations.empty() || !pRefKF) return;
  float normal[3] = {0.f, 0.f, 0.f};
  int n = 0;
  for (auto& o : observations) {
    const cv::Mat Owi = o.first->GetCameraCenter();
    float d[3];
    double s = 0;
    for (int k = 0; k < 3; k++) {
      d[k] = Pos.at<float>(k, 0) - Owi.at<float>(k, 0);
      s += (double)d[k] * d[k];
    }
    const double nrm = std::sqrt(s);  // cv::norm (L2, accumulated in double)
    for (int k = 0; k < 3; k++) normal[k] = normal[k] + (float)(d[k] / nrm);
    n++;
  }
  const cv::Mat Oref = pRefKF->GetCameraCenter();
  double s = 0;
  for (int k = 0; k < 3; k++) {
    const float d = Pos.at<float>(k, 0) - Oref.at<float>(k, 0);
    s += (double)d * d;
  }
  const float dist = (float)std::sqrt(s);
  const int level = pRefKF->mvKeysUn[observations[pRefKF]].octave;
  const float levelScaleFactor = pRefKF->mvScaleFactors[level];
  const int nLevels = pRefKF->mnScaleLevels;
  std::unique_lock<std::mutex> lock3(mMutexPos);
  mfMaxDistance = dist * levelScaleFactor;
  mfMinDistance = mfMaxDistance / pRefKF->mvScaleFactors[nLevels - 1];
  mNormalVector.create(3, 1, CV_32F);
  for (int k = 0; k < 3; k++) mNormalVector.at<float>(k, 0) = normal[k] / (float)n;
}

inline void MapPoint::Replace(MapPoint* pMP) {
  if (pMP->mnId == this->mnId) return;
  int nvisible, nfound;
  std::map<KeyFrame*, size_t> obs;
  {
    std::unique_lock<std::mutex> lock1(mMutexFeatures);
    std::unique_lock<std::mutex> lock2(mMutexPos);
    obs = mObservations;
    mObservations.clear();
    mbBad = true;
    nvisible = mnVisible;
    nfound = mnFound;
    mpReplaced = pMP;
  }
  for (auto& o : obs) {
    KeyFrame* pKF = o.first;
    if (!pMP->IsInKeyFrame(pKF)) {
      pKF->ReplaceMapPointMatch(o.second, pMP);
      pMP->AddObservation(pKF, o.second);
    } else {
      pKF->EraseMapPointMatch(o.second);
    }
  }
  pMP->IncreaseFound(nfound);
  pMP->IncreaseVisible(nvisible);
  pMP->ComputeDistinctiveDescriptors();
  if (mpMap) mpMap->EraseMapPoint(this);
}

inline void KeyFrame::UpdateBestCovisibles() {
  std::unique_lock<std::mutex> lock(mMutexConnections);
  std::vector<std::pair<std::pair<int, long unsigned int>, KeyFrame*>> vPairs;
  vPairs.reserve(mConnectedKeyFrameWeights.size());
  for (auto& m : mConnectedKeyFrameWeights) vPairs.push_back({{m.second, m.first->mnId}, m.first});
  std::sort(vPairs.begin(), vPairs.end());  // :180 (ascending weight; ascending mnId stands for the pointer)
  mvpOrderedConnectedKeyFrames.clear();
  mvOrderedWeights.clear();
  for (size_t i = vPairs.size(); i-- > 0;) {  // :183-187 push_front
    mvpOrderedConnectedKeyFrames.push_back(vPairs[i].second);
    mvOrderedWeights.push_back(vPairs[i].first.first);
  }
}

inline bool KeyFrame::SetBadFlagHost() {
  auto byId = [](KeyFrame* a, KeyFrame* b) { return a->mnId < b->mnId; };
  {
    std::unique_lock<std::mutex> lock(mMutexConnections);
    if (mnId == 0) return false;  // :571
    if (mbNotErase) {             // :573-577
      mbToBeErased = true;
      return false;
    }
  }
  {
    std::vector<KeyFrame*> conn;
    for (auto& m : mConnectedKeyFrameWeights) conn.push_back(m.first);
    for (KeyFrame* k : conn) k->EraseConnection(this);  // :581-582
  }
  for (size_t i = 0; i < mvpMapPoints.size(); i++)  // :585-587
    if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservation(this);
  KeyFrame* parent;
  std::vector<KeyFrame*> children;
  {
    std::unique_lock<std::mutex> lock(mMutexConnections);
    mConnectedKeyFrameWeights.clear();  // :593-594
    mvpOrderedConnectedKeyFrames.clear();
    parent = mpParent;
    children.assign(mspChildrens.begin(), mspChildrens.end());
  }
  std::sort(children.begin(), children.end(), byId);
  // Update Spanning Tree (:597-668): at each round the (child, candidate) pair of highest covisibility weight
  std::vector<KeyFrame*> sParentCandidates;
  if (parent) sParentCandidates.push_back(parent);
  while (!children.empty()) {
    bool bContinue = false;
    int max = -1;
    KeyFrame *pC = nullptr, *pP = nullptr;
    for (KeyFrame* pKF : children) {  // :612
      if (pKF->isBad()) continue;
      const std::vector<KeyFrame*> vpConnected = pKF->GetVectorCovisibleKeyFrames();
      for (size_t i = 0; i < vpConnected.size(); i++)
        for (KeyFrame* cand : sParentCandidates)  // :623 (ascending mnId)
          if (vpConnected[i]->mnId == cand->mnId) {
            const int w = pKF->GetWeight(vpConnected[i]);
            if (w > max) {
              pC = pKF;
              pP = vpConnected[i];
              max = w;
              bContinue = true;
            }
          }
    }
    if (!bContinue) break;
    pC->ChangeParent(pP);  // :651-655
    sParentCandidates.insert(std::upper_bound(sParentCandidates.begin(), sParentCandidates.end(), pC, byId), pC);
    children.erase(std::find(children.begin(), children.end(), pC));
  }
  if (parent) {
    for (KeyFrame* c : children) c->ChangeParent(parent);  // :663-668
    parent->EraseChild(this);                              // :670 (a keyframe without a parent skips it)
  }
  {
    std::unique_lock<std::mutex> lock(mMutexConnections);
    mspChildrens = std::set<KeyFrame*>(children.begin(), children.end());  // (the re-parented ones left at :655)
    mbBad = true;  // :672
  }
  if (mpMap) mpMap->EraseKeyFrame(this);  // :676
  return true;
}

inline void KeyFrame::SetPose(const cv::Mat& Tcw_) {
  std::unique_lock<std::mutex> lock(mMutexPose);
  Tcw_.copyTo(Tcw);
  Ow.create(3, 1, CV_32F);
  for (int r = 0; r < 3; r++) {  // Ow = -Rcw^T * tcw
    float acc = 0.f;
    for (int k = 0; k < 3; k++) acc += Tcw.at<float>(k, r) * Tcw.at<float>(k, 3);
    Ow.at<float>(r, 0) = -acc;
  }
}

class Frame {
 public:
  Frame() = default;
  // Stereo constructor, ORB part (src/Frame.cc:62-100, without timestamp / vocabulary / grid):
  // left and right extraction on two threads, N, the scale tables, the static intrinsics
  // (fx, fy, cx, cy, invfx, invfy from K, src/Frame.cc:111-126), mb = mbf/fx, UndistortKeyPoints
  // (a copy when mDistCoef(0) == 0, :473-476, else cv::undistortPoints on the GPU),
  // ComputeStereoMatches.  K: 3x3 CV_32F, distCoef: 4x1 or 5x1 CV_32F.
  Frame(const cv::Mat& imLeft, const cv::Mat& imRight, ORBextractor* extractorLeft, ORBextractor* extractorRight,
        const cv::Mat& K, const cv::Mat& distCoef, float bf, float thDepth);
  // The reference's stereo constructor with its own signature (include/Frame.h:55, src/Frame.cc:62-133):
  // as above, plus mnId / mTimeStamp / the vocabulary, mfLogScaleFactor, and on the first frame
  // ComputeImageBounds + the grid cell inverses (the statics mnMinX.., mfGridElementWidthInv..).
  Frame(const cv::Mat& imLeft, const cv::Mat& imRight, const double& timeStamp, ORBextractor* extractorLeft,
        ORBextractor* extractorRight, ORBVocabulary* voc, cv::Mat& K, cv::Mat& distCoef, const float& bf,
        const float& thDepth);

  // The reference's RGB-D constructor (include/Frame.h:58, src/Frame.cc:126-183): imGray CV_8UC1, imDepth
  // CV_32F as Tracking::GrabImageRGBD hands it over (already converted, src/Tracking.cc:230-231).
  // ExtractORB(0), UndistortKeyPoints and ComputeStereoFromRGBD run as ONE orbx_frame_rgbd call; fills
  // mvKeys, mDescriptors, mvKeysUn, mvuRight, mvDepth, the scale tables and mb, and on the first frame the
  // image bounds, the grid cell inverses and the static intrinsics.
  Frame(const cv::Mat& imGray, const cv::Mat& imDepth, const double& timeStamp, ORBextractor* extractor,
        ORBVocabulary* voc, cv::Mat& K, cv::Mat& distCoef, const float& bf, const float& thDepth);
  // The same with GrabImageRGBD's preprocessing inside the call (not in the reference): im may be CV_8UC1,
  // CV_8UC3 or CV_8UC4 (bRGB = Tracking's mbRGB: the byte order of a colour image), imDepth the RAW depth
  // image, CV_16U or CV_32F, and depthMapFactor Tracking's mDepthMapFactor (already inverted,
  // src/Tracking.cc:144-148).  The caller skips cvtColor and the host convertTo: the conversion is applied
  // to the pixels under the keypoints, under the reference's condition (:230).
  Frame(const cv::Mat& im, const cv::Mat& imDepth, const double& timeStamp, ORBextractor* extractor,
        ORBVocabulary* voc, cv::Mat& K, cv::Mat& distCoef, const float& bf, const float& thDepth,
        const float& depthMapFactor, bool bRGB = true);
  // The reference's monocular constructor (include/Frame.h:61, src/Frame.cc:186-251): extraction and
  // undistortion, mvuRight and mvDepth all -1.
  Frame(const cv::Mat& imGray, const double& timeStamp, ORBextractor* extractor, ORBVocabulary* voc, cv::Mat& K,
        cv::Mat& distCoef, const float& bf, const float& thDepth);

  void ExtractORB(int flag, const cv::Mat& im);  // src/Frame.cc:273-279
  // src/Frame.cc:791-816 on a CV_32F depth image, from mvKeys / mvKeysUn / mbf (the constructors above get
  // the same values from the GPU inside orbx_frame_rgbd; this member is the reference's own loop, for
  // callers that invoke it on its own)
  void ComputeStereoFromRGBD(const cv::Mat& imDepth);
  void UndistortKeyPoints();                     // src/Frame.cc:471-506
  void ComputeImageBounds(const cv::Mat& imLeft);  // src/Frame.cc:508-537 (corners on the MI355X)
  void ComputeStereoMatches();                   // src/Frame.cc:547-788 (on the MI355X)
  void ComputeBoW();                             // src/Frame.cc:462-469 (ORBVocabulary::transform on the MI355X)
  void SetPose(const cv::Mat& Tcw);              // src/Frame.cc SetPose + UpdatePoseMatrices
  void UpdatePoseMatrices();
  cv::Mat GetCameraCenter() { return mOw.clone(); }

  cv::Mat mK, mDistCoef;
  static float fx, fy, cx, cy, invfx, invfy;  // include/Frame.h:135-140
  // image bounds and grid cell inverses, computed once (include/Frame.h: static float mnMinX ...)
  static float mnMinX, mnMaxX, mnMinY, mnMaxY;
  static float mfGridElementWidthInv, mfGridElementHeightInv;
  static bool mbInitialComputations;
  ORBVocabulary* mpORBvocabulary = nullptr;
  DBoW2::BowVector mBowVec;
  double mTimeStamp = 0.0;
  static long unsigned int nNextId;
  long unsigned int mnId = 0;
  cv::Mat mTcw, mRcw, mtcw, mRwc, mOw;
  float mfLogScaleFactor = 0.f;

  ORBextractor* mpORBextractorLeft = nullptr;
  ORBextractor* mpORBextractorRight = nullptr;
  float mbf = 0.f, mb = 0.f, mThDepth = 0.f;
  int N = 0;
  std::vector<cv::KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
  std::vector<float> mvuRight, mvDepth;
  cv::Mat mDescriptors, mDescriptorsRight;
  DBoW2::FeatureVector mFeatVec;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  int mnScaleLevels = 0;
  float mfScaleFactor = 0.f;
  std::vector<float> mvScaleFactors, mvInvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;

 private:
  // src/Frame.cc:86-123 after the two ExtractORB calls; uR / dep: stereo results already computed by
  // orbx_frame_stereo (null: ComputeStereoMatches runs)
  void finish_stereo_frame(const std::vector<float>* uR, const std::vector<float>* dep);
  // the RGB-D (imDepth non-null) and monocular (null) constructors' shared body, src/Frame.cc:130-183, 190-251
  void init_single_camera(const cv::Mat& im, const cv::Mat* imDepth, float depthMapFactor, bool bRGB,
                          const double& timeStamp, ORBVocabulary* voc);
};

// Free-function form of Frame::ComputeStereoMatches for callers without a Frame object:
// mvuRight / mvDepth (resized to kpsL.size()) from two extractors' last extraction.
void ComputeStereoMatches(ORBextractor& left, ORBextractor& right, const std::vector<cv::KeyPoint>& kpsL,
                          const cv::Mat& descL, const std::vector<cv::KeyPoint>& kpsR, const cv::Mat& descR,
                          float mbf, float mb, std::vector<float>& mvuRight, std::vector<float>& mvDepth);

}  // namespace ORB_SLAM2

// KeyFrameDatabase.h -- drop-in ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h,
// src/KeyFrameDatabase.cc:33-341) over orbx_kfdb_*: the inverted file and both candidate queries live
// on the MI355X.  A KeyFrame is known to the device by its mnId.  Before a query the neighbour lists
// (GetBestCovisibilityKeyFrames(10)) of the database's keyframes are uploaded in one call; after it
// the six members the reference's queries write (mnRelocQuery, mnRelocWords, mRelocScore, mnLoopQuery,
// mnLoopWords, mLoopScore) are written back into the database's KeyFrames, so code that reads them
// sees the reference's values.
#pragma once
#include <map>
#include <mutex>
#include <vector>

#include "ORBVocabulary.h"
#include "Objects.h"
#include "orbx.h"

namespace ORB_SLAM2 {

class KeyFrameDatabase {
 public:
  KeyFrameDatabase(const ORBVocabulary& voc);
  ~KeyFrameDatabase();
  KeyFrameDatabase(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

  void add(KeyFrame* pKF);
  void erase(KeyFrame* pKF);
  void clear();

  // Loop Detection
  std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore);
  // Relocalization
  std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F);

  orbx_kfdb* gpu() const { return mpGpu; }

 protected:
  void UploadNeighbours();
  void WriteBackState();
  std::vector<KeyFrame*> ToKeyFrames(const std::vector<int64_t>& ids) const;

  const ORBVocabulary* mpVoc;
  orbx_kfdb* mpGpu = nullptr;
  std::map<long unsigned int, KeyFrame*> mKeyFrames;  // the keyframes in the database, by mnId
  std::mutex mMutex;
};

}  // namespace ORB_SLAM2

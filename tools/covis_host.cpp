// covis_host.cpp -- the host side of tools/covis_time.py: the covisibility queries the way the reference runs
// them, nested std::map<KeyFrame*, ...> walks keyframe by point by observation (src/KeyFrame.cc:367-467,
// src/Tracking.cc:1483-1581, src/LocalMapping.cc:784-871, src/MapPoint.cc:98-170), behind a small C interface
// with the same arguments as the orbx_covis_* calls so that both sides are timed on the same inputs.  A
// straightforward restatement for timing; the yardstick for correctness is tests/covis_literal.py.
#include <algorithm>
#include <cstdint>
#include <list>
#include <map>
#include <memory>
#include <set>
#include <vector>

namespace {

struct KF;
struct MP {
  int32_t id = 0;
  std::map<KF*, size_t> mObservations;
  int nObs = 0;
  bool mbBad = false;
  long mnTrackReferenceForFrame = -1;
};
struct KF {
  int64_t mnId = 0;
  std::vector<MP*> mvpMapPoints;
  std::vector<int> octave;
  std::vector<uint8_t> flags;  // 1 stereo, 2 close
  bool live = true;
};
struct World {
  std::map<int64_t, std::unique_ptr<KF>> kfs;
  std::map<int32_t, std::unique_ptr<MP>> mps;
  long frame = 0;
  MP* mp(int32_t id) {
    std::unique_ptr<MP>& p = mps[id];
    if (!p) {
      p.reset(new MP());
      p->id = id;
    }
    return p.get();
  }
};

void set_bad(MP* p) {  // src/MapPoint.cc:153-170
  p->mbBad = true;
  std::map<KF*, size_t> obs = p->mObservations;
  p->mObservations.clear();
  for (auto& o : obs) o.first->mvpMapPoints[o.second] = nullptr;
}

void erase_observation(MP* p, KF* k) {  // src/MapPoint.cc:113-139
  auto it = p->mObservations.find(k);
  if (it == p->mObservations.end()) return;
  p->nObs -= (k->flags[it->second] & 1) ? 2 : 1;
  p->mObservations.erase(it);
  if (p->nObs <= 2) set_bad(p);
}

}  // namespace

extern "C" {

void* covis_host_create() { return new World(); }
void covis_host_destroy(void* h) { delete (World*)h; }

void covis_host_set_keyframe(void* h, int64_t id, int n, const int32_t* pid, const int32_t* oct, const uint8_t* fl) {
  World* W = (World*)h;
  std::unique_ptr<KF>& k = W->kfs[id];
  if (!k) {
    k.reset(new KF());
    k->mnId = id;
  }
  for (size_t i = 0; i < k->mvpMapPoints.size(); i++)
    if (MP* p = k->mvpMapPoints[i]) {
      auto it = p->mObservations.find(k.get());
      if (it != p->mObservations.end()) {
        p->nObs -= (k->flags[i] & 1) ? 2 : 1;
        p->mObservations.erase(it);
      }
    }
  k->live = true;
  k->mvpMapPoints.assign(n, nullptr);
  k->octave.assign(oct, oct + n);
  k->flags.assign(fl, fl + n);
  for (int i = 0; i < n; i++) {
    if (pid[i] < 0) continue;
    MP* p = W->mp(pid[i]);
    if (p->mbBad) continue;
    k->mvpMapPoints[i] = p;
    p->mObservations[k.get()] = i;  // src/MapPoint.cc:98-111
    p->nObs += (fl[i] & 1) ? 2 : 1;
  }
}

// UpdateConnections steps 1-2: returns KFcounter.size(); *n_ordered the ordered list's length, *first its head
int covis_host_update_connections(void* h, int64_t id, int th, int* n_ordered, int64_t* first) {
  World* W = (World*)h;
  KF* self = W->kfs[id].get();
  std::map<KF*, int> KFcounter;
  for (MP* pMP : self->mvpMapPoints) {
    if (!pMP || pMP->mbBad) continue;
    std::map<KF*, size_t> observations = pMP->mObservations;  // GetObservations() copies
    for (auto& o : observations) {
      if (o.first->mnId == self->mnId) continue;
      KFcounter[o.first]++;
    }
  }
  *n_ordered = 0;
  *first = -1;
  if (KFcounter.empty()) return 0;
  int nmax = 0;
  KF* pKFmax = nullptr;
  std::vector<std::pair<int, int64_t>> vPairs;
  vPairs.reserve(KFcounter.size());
  for (auto& m : KFcounter) {
    if (m.second > nmax) {
      nmax = m.second;
      pKFmax = m.first;
    }
    if (m.second >= th) vPairs.push_back({m.second, m.first->mnId});
  }
  if (vPairs.empty()) vPairs.push_back({nmax, pKFmax->mnId});
  std::sort(vPairs.begin(), vPairs.end());
  std::list<int64_t> lKFs;
  std::list<int> lWs;
  for (auto& p : vPairs) {
    lKFs.push_front(p.second);
    lWs.push_front(p.first);
  }
  *n_ordered = (int)lKFs.size();
  *first = lKFs.front();
  return (int)KFcounter.size();
}

// the vote of UpdateLocalKeyFrames: returns keyframeCounter.size(), *kf_max pKFmax
int covis_host_vote(void* h, const int32_t* pid, int n, int64_t* kf_max) {
  World* W = (World*)h;
  std::map<KF*, int> keyframeCounter;
  for (int i = 0; i < n; i++) {
    if (pid[i] < 0) continue;
    auto it = W->mps.find(pid[i]);
    if (it == W->mps.end()) continue;
    MP* pMP = it->second.get();
    if (pMP->mbBad) continue;
    const std::map<KF*, size_t> observations = pMP->mObservations;
    for (auto& o : observations) keyframeCounter[o.first]++;
  }
  int max = 0;
  *kf_max = -1;
  // (std::map<KF*, ..> walks in pointer order; the timing does not depend on which of the maxima wins)
  for (auto& m : keyframeCounter)
    if (m.second > max) {
      max = m.second;
      *kf_max = m.first->mnId;
    }
  return (int)keyframeCounter.size();
}

int covis_host_local_points(void* h, const int64_t* ids, int n, int32_t* out) {
  World* W = (World*)h;
  const long frame = ++W->frame;
  int m = 0;
  for (int k = 0; k < n; k++) {
    const std::vector<MP*> vpMPs = W->kfs[ids[k]]->mvpMapPoints;  // GetMapPointMatches() copies
    for (MP* pMP : vpMPs) {
      if (!pMP) continue;
      if (pMP->mnTrackReferenceForFrame == frame) continue;
      if (!pMP->mbBad) {
        out[m++] = pMP->id;
        pMP->mnTrackReferenceForFrame = frame;
      }
    }
  }
  return m;
}

// KeyFrameCulling with the observation half of SetBadFlag: verdict per candidate (0 kept, 1 culled, 2 held)
void covis_host_cull(void* h, const int64_t* ids, int n, const uint8_t* not_erase, int monocular, uint8_t* verdict) {
  World* W = (World*)h;
  for (int c = 0; c < n; c++) {
    KF* pKF = W->kfs[ids[c]].get();
    verdict[c] = 0;
    if (pKF->mnId == 0) continue;
    const std::vector<MP*> vpMapPoints = pKF->mvpMapPoints;
    const int thObs = 3;
    int nRedundantObservations = 0, nMPs = 0;
    for (size_t i = 0; i < vpMapPoints.size(); i++) {
      MP* pMP = vpMapPoints[i];
      if (!pMP || pMP->mbBad) continue;
      if (!monocular && !(pKF->flags[i] & 2)) continue;
      nMPs++;
      if (pMP->nObs > thObs) {
        const int scaleLevel = pKF->octave[i];
        const std::map<KF*, size_t> observations = pMP->mObservations;
        int nObs = 0;
        for (auto& o : observations) {
          if (o.first == pKF) continue;
          if (o.first->octave[o.second] <= scaleLevel + 1) {
            nObs++;
            if (nObs >= thObs) break;
          }
        }
        if (nObs >= thObs) nRedundantObservations++;
      }
    }
    if (nRedundantObservations > 0.9 * nMPs) {
      if (not_erase[c]) {
        verdict[c] = 2;
        continue;
      }
      verdict[c] = 1;
      for (size_t i = 0; i < pKF->mvpMapPoints.size(); i++)
        if (pKF->mvpMapPoints[i]) erase_observation(pKF->mvpMapPoints[i], pKF);
      pKF->live = false;
      pKF->mvpMapPoints.clear();
    }
  }
}

}  // extern "C"

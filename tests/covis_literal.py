"""A literal Python restatement of the reference's covisibility bookkeeping -- the yardstick of
tests/test_covis.py and tests/test_covis_shim.py.  It is not the code under test and needs no GPU.

A small object model (KeyFrame: mvpMapPoints, octaves, mvuRight, mvDepth, mConnectedKeyFrameWeights, the
ordered vectors, parent and children; MapPoint: mObservations, nObs, mbBad) and, line by line with the
reference's line numbers:

  KeyFrame.AddConnection / UpdateBestCovisibles / EraseConnection   src/KeyFrame.cc:147-192, 686-700
  KeyFrame.UpdateConnections                                        src/KeyFrame.cc:367-493
  KeyFrame.SetBadFlag                                               src/KeyFrame.cc:567-678
  MapPoint.AddObservation / EraseObservation / SetBadFlag           src/MapPoint.cc:98-170
  KeyFrameCulling                                                   src/LocalMapping.cc:784-871
  UpdateLocalKeyFrames (first half) / UpdateLocalPoints             src/Tracking.cc:1518-1581, 1483-1515

Every std::map<KeyFrame*, ..> and std::set<KeyFrame*> is walked in ascending mnId, which stands for
pointer order as everywhere in this project.  Not restated: mpRefKF (src/MapPoint.cc:128-129), mTcp
(src/KeyFrame.cc:671), the Map and KeyFrameDatabase erasures (:676-677) beyond dropping the keyframe from
the table.  A keyframe without a parent skips :670 (the reference would dereference NULL; only keyframe 0
and keyframes that never ran UpdateConnections are in that state).

Table (the `Table` class) holds what the library's handle holds: the live keyframes and every point seen.
Its set_keyframe / erase_keyframe / set_points_bad are the three calls of include/orbx.h stated on the
objects: a row put in adds its observations, a row taken out removes them without the nObs <= 2 test (only
KeyFrameCulling's EraseObservation and set_points_bad turn points bad), a bad point is never observed
again.
"""

STEREO, CLOSE = 1, 2
TH_DEPTH = 2.0


def by_id(items):
    """A std::map / std::set keyed by KeyFrame* in its iteration order."""
    if isinstance(items, dict):
        return sorted(items.items(), key=lambda kv: kv[0].mnId)
    return sorted(items, key=lambda k: k.mnId)


class MapPoint:
    def __init__(self, mnId, table=None):
        self.mnId = mnId
        self.mObservations = {}  # KeyFrame -> idx
        self.nObs = 0
        self.mbBad = False
        self.mnTrackReferenceForFrame = 0
        self.table = table

    def isBad(self):
        return self.mbBad

    def Observations(self):
        return self.nObs

    def GetObservations(self):
        return dict(self.mObservations)

    def AddObservation(self, pKF, idx):  # src/MapPoint.cc:98-111
        if pKF in self.mObservations:
            return
        self.mObservations[pKF] = idx
        if pKF.mvuRight[idx] >= 0:
            self.nObs += 2
        else:
            self.nObs += 1

    def EraseObservation(self, pKF):  # src/MapPoint.cc:113-139
        bBad = False
        if pKF in self.mObservations:             # :118
            idx = self.mObservations[pKF]         # :120
            if pKF.mvuRight[idx] >= 0:            # :121
                self.nObs -= 2
            else:
                self.nObs -= 1
            del self.mObservations[pKF]           # :126
            if self.nObs <= 2:                    # :132
                bBad = True
        if bBad:
            self.SetBadFlag()                     # :138

    def SetBadFlag(self):  # src/MapPoint.cc:153-170
        was = self.mbBad
        self.mbBad = True                         # :159
        obs = self.mObservations                  # :160
        self.mObservations = {}                   # :161
        for pKF, idx in by_id(obs):               # :163-167
            pKF.EraseMapPointMatch(idx)
        if self.table is not None and not was:
            self.table.went_bad.append(self.mnId)


class KeyFrame:
    def __init__(self, mnId, table=None):
        self.mnId = mnId
        self.table = table
        self.mvpMapPoints = []
        self.octaves = []      # mvKeysUn[i].octave
        self.mvuRight = []
        self.mvDepth = []
        self.mThDepth = TH_DEPTH
        self.mConnectedKeyFrameWeights = {}
        self.mvpOrderedConnectedKeyFrames = []
        self.mvOrderedWeights = []
        self.mbFirstConnection = True
        self.mpParent = None
        self.mspChildrens = set()
        self.mbNotErase = False
        self.mbToBeErased = False
        self.mbBad = False
        self.mnTrackReferenceForFrame = 0

    def isBad(self):
        return self.mbBad

    def EraseMapPointMatch(self, idx):
        self.mvpMapPoints[idx] = None

    def GetMapPointMatches(self):
        return list(self.mvpMapPoints)

    def GetVectorCovisibleKeyFrames(self):
        return list(self.mvpOrderedConnectedKeyFrames)

    def GetWeight(self, pKF):  # src/KeyFrame.cc:261-268
        return self.mConnectedKeyFrameWeights.get(pKF, 0)

    def AddChild(self, pKF):
        self.mspChildrens.add(pKF)

    def EraseChild(self, pKF):
        self.mspChildrens.discard(pKF)

    def ChangeParent(self, pKF):  # src/KeyFrame.cc:507-512
        self.mpParent = pKF
        pKF.AddChild(self)

    def AddConnection(self, pKF, weight):  # src/KeyFrame.cc:147-162
        if pKF not in self.mConnectedKeyFrameWeights:          # :152
            self.mConnectedKeyFrameWeights[pKF] = weight
        elif self.mConnectedKeyFrameWeights[pKF] != weight:    # :154
            self.mConnectedKeyFrameWeights[pKF] = weight
        else:
            return
        self.UpdateBestCovisibles()                            # :161

    def UpdateBestCovisibles(self):  # src/KeyFrame.cc:169-192
        vPairs = [(w, k) for k, w in by_id(self.mConnectedKeyFrameWeights)]  # :176-177
        vPairs.sort(key=lambda t: (t[0], t[1].mnId))                         # :180
        lKFs, lWs = [], []
        for w, k in vPairs:                                                  # :183-187 push_front
            lKFs.insert(0, k)
            lWs.insert(0, w)
        self.mvpOrderedConnectedKeyFrames = lKFs                             # :190
        self.mvOrderedWeights = lWs

    def EraseConnection(self, pKF):  # src/KeyFrame.cc:686-700
        bUpdate = False
        if pKF in self.mConnectedKeyFrameWeights:
            del self.mConnectedKeyFrameWeights[pKF]
            bUpdate = True
        if bUpdate:
            self.UpdateBestCovisibles()

    def UpdateConnections(self, th=15):  # src/KeyFrame.cc:367-493 (th: the reference's 15, :424)
        """Returns (KFcounter as [(id, count)] ascending, vPairs as [(id, weight)] in the final order), both
        empty when :414 returns early."""
        KFcounter = {}                                      # :373
        vpMP = list(self.mvpMapPoints)                      # :381
        for pMP in vpMP:                                    # :388
            if pMP is None:                                 # :392
                continue
            if pMP.isBad():                                 # :395
                continue
            observations = pMP.GetObservations()            # :398
            for pKFi, _ in by_id(observations):             # :401
                if pKFi.mnId == self.mnId:                  # :405
                    continue
                KFcounter[pKFi] = KFcounter.get(pKFi, 0) + 1  # :408
        if not KFcounter:                                   # :414
            return [], []
        nmax, pKFmax = 0, None                              # :421-422
        vPairs = []
        for pKFi, n in by_id(KFcounter):                    # :430
            if n > nmax:                                    # :434
                nmax, pKFmax = n, pKFi
            if n >= th:                                     # :440
                vPairs.append((n, pKFi))
                pKFi.AddConnection(self, n)                 # :445
        if not vPairs:                                      # :450
            vPairs.append((nmax, pKFmax))
            pKFmax.AddConnection(self, nmax)                # :455
        vPairs.sort(key=lambda t: (t[0], t[1].mnId))        # :459
        lKFs, lWs = [], []
        for w, k in vPairs:                                 # :463-467
            lKFs.insert(0, k)
            lWs.insert(0, w)
        self.mConnectedKeyFrameWeights = dict(KFcounter)    # :475
        self.mvpOrderedConnectedKeyFrames = lKFs            # :478
        self.mvOrderedWeights = lWs                         # :479
        if self.mbFirstConnection and self.mnId != 0:       # :482
            self.mpParent = self.mvpOrderedConnectedKeyFrames[0]  # :486
            self.mpParent.AddChild(self)                    # :488
            self.mbFirstConnection = False                  # :489
        return ([(k.mnId, n) for k, n in by_id(KFcounter)], [(k.mnId, w) for k, w in zip(lKFs, lWs)])

    def SetBadFlag(self):  # src/KeyFrame.cc:567-678
        if self.mnId == 0:                                  # :571
            return
        elif self.mbNotErase:                               # :573
            self.mbToBeErased = True
            return
        for pKFi, _ in by_id(self.mConnectedKeyFrameWeights):  # :581-582
            pKFi.EraseConnection(self)
        for pMP in list(self.mvpMapPoints):                 # :585-587
            if pMP is not None:
                pMP.EraseObservation(self)
        self.mConnectedKeyFrameWeights = {}                 # :593
        self.mvpOrderedConnectedKeyFrames = []              # :594
        sParentCandidates = set()                           # :597-598
        if self.mpParent is not None:
            sParentCandidates.add(self.mpParent)
        while self.mspChildrens:                            # :603
            bContinue = False
            mx, pC, pP = -1, None, None
            for pKF in by_id(self.mspChildrens):            # :612
                if pKF.isBad():                             # :615
                    continue
                vpConnected = pKF.GetVectorCovisibleKeyFrames()  # :620
                for pCon in vpConnected:                    # :621
                    for pCand in by_id(sParentCandidates):  # :623
                        if pCon.mnId == pCand.mnId:         # :633
                            w = pKF.GetWeight(pCon)         # :635
                            if w > mx:                      # :636
                                pC, pP, mx = pKF, pCon, w
                                bContinue = True
            if bContinue:                                   # :648
                pC.ChangeParent(pP)                         # :651
                sParentCandidates.add(pC)                   # :653
                self.mspChildrens.discard(pC)               # :655
            else:
                break
        if self.mspChildrens and self.mpParent is not None:  # :663-668
            for pKF in by_id(self.mspChildrens):
                pKF.ChangeParent(self.mpParent)
        if self.mpParent is not None:
            self.mpParent.EraseChild(self)                  # :670
        self.mbBad = True                                   # :672
        if self.table is not None:                          # :676-677
            self.table.kfs.pop(self.mnId, None)


def KeyFrameCulling(vpLocalKeyFrames, mbMonocular, trace=None):  # src/LocalMapping.cc:784-871
    """vpLocalKeyFrames = mpCurrentKeyFrame->GetVectorCovisibleKeyFrames() (:793).  Returns the verdict per
    candidate: 0 kept, 1 culled (SetBadFlag ran), 2 to be erased (mbNotErase held it).  trace, when a list,
    receives (mnId, nMPs, nRedundantObservations) per judged candidate."""
    verdicts = []
    for pKF in vpLocalKeyFrames:                            # :796
        if pKF.mnId == 0:                                   # :799
            verdicts.append(0)
            continue
        vpMapPoints = pKF.GetMapPointMatches()              # :802
        thObs = 3                                           # :804-805
        nRedundantObservations = 0
        nMPs = 0
        for i, pMP in enumerate(vpMapPoints):               # :810
            if pMP is not None:                             # :813
                if not pMP.isBad():                         # :815
                    if not mbMonocular:                     # :818
                        if pKF.mvDepth[i] > pKF.mThDepth or pKF.mvDepth[i] < 0:  # :820
                            continue
                    nMPs += 1                               # :824
                    if pMP.Observations() > thObs:          # :826
                        scaleLevel = pKF.octaves[i]         # :830
                        observations = pMP.GetObservations()  # :832
                        nObs = 0
                        for pKFi, idx in by_id(observations):  # :834
                            if pKFi is pKF:                 # :841
                                continue
                            scaleLeveli = pKFi.octaves[idx]  # :844
                            if scaleLeveli <= scaleLevel + 1:  # :847
                                nObs += 1
                                if nObs >= thObs:           # :851
                                    break
                        if nObs >= thObs:                   # :857
                            nRedundantObservations += 1
        if trace is not None:
            trace.append((pKF.mnId, nMPs, nRedundantObservations))
        if nRedundantObservations > 0.9 * nMPs:             # :868
            pKF.SetBadFlag()                                # :869
            verdicts.append(2 if pKF.mbToBeErased and not pKF.mbBad else 1)
        else:
            verdicts.append(0)
    return verdicts


def UpdateLocalKeyFrames(frame_points):  # src/Tracking.cc:1518-1581 (the vote)
    """frame_points: mCurrentFrame.mvpMapPoints (MapPoint or None), nulled in place as :1540 does.  Returns
    (keyframeCounter as [(id, count)] ascending, pKFmax id or None, max)."""
    keyframeCounter = {}                                    # :1523
    for i in range(len(frame_points)):                      # :1524
        if frame_points[i] is not None:                     # :1527
            pMP = frame_points[i]
            if not pMP.isBad():                             # :1530
                for pKF, _ in by_id(pMP.GetObservations()):  # :1534-1536
                    keyframeCounter[pKF] = keyframeCounter.get(pKF, 0) + 1
            else:
                frame_points[i] = None                      # :1540
    if not keyframeCounter:                                 # :1547
        return [], None, 0
    mx, pKFmax = 0, None                                    # :1550-1551
    for pKF, n in by_id(keyframeCounter):                   # :1560
        if pKF.isBad():                                     # :1565
            continue
        if n > mx:                                          # :1570
            mx, pKFmax = n, pKF
    return [(k.mnId, n) for k, n in by_id(keyframeCounter)], (None if pKFmax is None else pKFmax.mnId), mx


def UpdateLocalPoints(mvpLocalKeyFrames, frame_id):  # src/Tracking.cc:1483-1515
    mvpLocalMapPoints = []                                  # :1486
    for pKF in mvpLocalKeyFrames:                           # :1489
        vpMPs = pKF.GetMapPointMatches()                    # :1493
        for pMP in vpMPs:                                   # :1496
            if pMP is None:                                 # :1499
                continue
            if pMP.mnTrackReferenceForFrame == frame_id:    # :1503
                continue
            if not pMP.isBad():                             # :1506
                mvpLocalMapPoints.append(pMP)               # :1509
                pMP.mnTrackReferenceForFrame = frame_id     # :1511
    return [p.mnId for p in mvpLocalMapPoints]


def flags_to_stereo_depth(f):
    """mvuRight / mvDepth values that give the two flag bits under mThDepth = TH_DEPTH."""
    return (1.0 if f & STEREO else -1.0), (1.0 if f & CLOSE else (3.0 if f & STEREO else -1.0))


class Table:
    """The live keyframes and every point seen, with the handle's three mutating calls."""

    def __init__(self):
        self.kfs = {}
        self.points = {}
        self.went_bad = []
        self.frame_id = 0

    def point(self, pid):
        if pid not in self.points:
            self.points[pid] = MapPoint(pid, self)
        return self.points[pid]

    def _take_out(self, kf):
        for idx, pMP in enumerate(kf.mvpMapPoints):
            if pMP is not None and not pMP.mbBad and kf in pMP.mObservations:
                pMP.nObs -= 2 if kf.mvuRight[idx] >= 0 else 1
                del pMP.mObservations[kf]

    def set_keyframe(self, kf_id, entries):
        """entries: [(point id or -1, octave, flags)]."""
        kf = self.kfs.get(kf_id)
        if kf is None:
            kf = self.kfs[kf_id] = KeyFrame(kf_id, self)
        else:
            self._take_out(kf)
        kf.octaves = [e[1] for e in entries]
        kf.flags = [e[2] for e in entries]
        sd = [flags_to_stereo_depth(e[2]) for e in entries]
        kf.mvuRight = [s for s, _ in sd]
        kf.mvDepth = [d for _, d in sd]
        kf.mvpMapPoints = [None] * len(entries)
        for idx, e in enumerate(entries):
            if e[0] < 0:
                continue
            pMP = self.point(e[0])
            if pMP.mbBad:
                continue  # a bad point is observed by nobody: the slot is what EraseMapPointMatch leaves
            kf.mvpMapPoints[idx] = pMP
            pMP.AddObservation(kf, idx)
        return kf

    def erase_keyframe(self, kf_id):
        self._take_out(self.kfs.pop(kf_id))

    def set_points_bad(self, ids):
        for pid in ids:
            self.point(pid).SetBadFlag()

    def state(self):
        """({kf: (point ids, octaves, flags)}, {point: (nObs, bad)}) as the read-back probes return them."""
        rows = {k: ([-1 if p is None else p.mnId for p in kf.mvpMapPoints], list(kf.octaves), list(kf.flags))
                for k, kf in self.kfs.items()}
        pts = {i: (p.nObs, int(p.mbBad)) for i, p in self.points.items()}
        return rows, pts

    # the four queries, on ids
    def update_connections(self, kf_id, th=15):
        return self.kfs[kf_id].UpdateConnections(th)

    def vote(self, point_ids):
        fp = [None if i < 0 else self.points.get(i) for i in point_ids]
        before = list(fp)
        counter, kmax, mx = UpdateLocalKeyFrames(fp)
        was_bad = [int(b is not None and a is None) for a, b in zip(fp, before)]
        return was_bad, counter, kmax, mx

    def local_points(self, kf_ids):
        self.frame_id += 1
        return UpdateLocalPoints([self.kfs[k] for k in kf_ids], self.frame_id)

    def cull(self, cand_ids, not_erase, monocular, trace=None):
        cands = [self.kfs[k] for k in cand_ids]
        for k, ne in zip(cands, not_erase):
            k.mbNotErase = bool(ne)
        self.went_bad = []
        v = KeyFrameCulling(cands, monocular, trace)
        return v, sorted(self.went_bad)

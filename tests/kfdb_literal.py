"""A literal Python restatement of the reference's KeyFrameDatabase (src/KeyFrameDatabase.cc:33-341)
and of DBoW2's L1Scoring::score -- the yardstick of tests/test_kfdb.py and tests/test_kfdb_shim.py.

Lists and sets as in the reference, one small object per keyframe with the six members the queries
touch, np.float32 wherever the reference has `float`, Python floats (doubles) for score.  It is not
the code under test and needs no GPU.  `counters` records how often each quirk branch fired, so a
test can assert that its input reaches the branch it is about.

Choices shared with the library (include/orbx.h): mnRelocQuery / mnLoopQuery / mn*Words start at 0
(src/KeyFrame.cc:35), mRelocScore / mLoopScore (uninitialised in the reference) start at 0.0f, a
keyframe object lives as long as its id has ever been seen, and a neighbour that is not in the
database at query time is skipped.
"""
import collections

import numpy as np

F32 = np.float32


def score(v, w):
    """L1Scoring::score(v, w) on BowVectors given as (words, values) with ascending words:
    both are walked like the std::map iterators, the common words met in ascending order."""
    vw, vv = v
    ww, wv = w
    i = j = 0
    s = 0.0
    while i < len(vw) and j < len(ww):
        if vw[i] == ww[j]:
            vi, wi = float(vv[i]), float(wv[j])
            s += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif vw[i] < ww[j]:
            i += 1  # lower_bound in the original: same visits
        else:
            j += 1
    return -s / 2.0


def score_terms(v, w):
    """The addends of score() in the order it adds them."""
    wmap = {int(k): float(x) for k, x in zip(*w)}
    out = []
    for k, x in zip(*v):
        if int(k) in wmap:
            vi, wi = float(x), wmap[int(k)]
            out.append(abs(vi - wi) - abs(vi) - abs(wi))
    return out


class KeyFrame:
    def __init__(self, mnId):
        self.mnId = mnId
        self.mBowVec = (np.zeros(0, np.uint32), np.zeros(0, np.float64))
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = F32(0.0)
        self.mnLoopQuery = 0
        self.mnLoopWords = 0
        self.mLoopScore = F32(0.0)
        self.best10 = []  # ids, GetBestCovisibilityKeyFrames(10)

    def state(self):
        return (self.mnRelocQuery, self.mnRelocWords, F32(self.mRelocScore), self.mnLoopQuery, self.mnLoopWords,
                F32(self.mLoopScore))


class KeyFrameDatabase:
    def __init__(self, n_words):
        self.n_words = n_words
        self.mvInvertedFile = collections.defaultdict(list)
        self.kfs = {}       # every id ever seen
        self.live = set()
        self.counters = collections.Counter()

    def kf(self, mnId):
        if mnId not in self.kfs:
            self.kfs[mnId] = KeyFrame(mnId)
        return self.kfs[mnId]

    def add(self, mnId, bow):
        assert mnId not in self.live
        pKF = self.kf(mnId)
        pKF.mBowVec = (np.asarray(bow[0]).copy(), np.asarray(bow[1]).copy())
        for w in pKF.mBowVec[0]:
            self.mvInvertedFile[int(w)].append(pKF)
        self.live.add(mnId)

    def erase(self, mnId):
        if mnId not in self.live:
            return
        pKF = self.kfs[mnId]
        for w in pKF.mBowVec[0]:
            lKFs = self.mvInvertedFile[int(w)]
            for k, x in enumerate(lKFs):
                if x is pKF:
                    del lKFs[k]
                    break
        self.live.discard(mnId)

    def clear(self):
        self.mvInvertedFile.clear()
        self.kfs.clear()
        self.live.clear()

    def set_neighbours(self, mnId, best10):
        assert len(best10) <= 10
        self.kf(mnId).best10 = [int(x) for x in best10]
        for x in best10:
            self.kf(int(x))

    def _neighbours(self, pKFi):
        out = []
        for x in pKFi.best10:
            if x in self.live:
                out.append(self.kfs[x])
            else:
                self.counters["neighbour_not_live"] += 1
        return out

    def score(self, bow, mnId):
        return score(bow, self.kfs[mnId].mBowVec)

    # src/KeyFrameDatabase.cc:219-341
    def DetectRelocalizationCandidates(self, F_mnId, F_bow):
        C = self.counters
        lKFsSharingWords = []
        listed = set()  # ids in lKFsSharingWords (bookkeeping for the counter only)
        for w in F_bow[0]:
            for pKFi in self.mvInvertedFile.get(int(w), ()):
                if pKFi.mnRelocQuery != F_mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F_mnId
                    lKFsSharingWords.append(pKFi)
                    listed.add(pKFi.mnId)
                elif pKFi.mnId not in listed:
                    C["reloc_same_id_counts_up"] += 1
                pKFi.mnRelocWords += 1
        if not lKFsSharingWords:
            C["reloc_nothing_shared"] += 1
            return []
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > maxCommonWords:
                maxCommonWords = pKFi.mnRelocWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        self.last_min_common = minCommonWords
        lScoreAndMatch = []
        scored = set()
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(score(F_bow, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
                scored.add(pKFi.mnId)
            else:
                C["reloc_not_scored"] += 1
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):
                if pKF2.mnRelocQuery != F_mnId:
                    continue
                if pKF2.mnId not in scored:
                    C["reloc_stale_score_accumulated"] += 1
                accScore = F32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
                    if pKF2.mnId not in scored:
                        C["reloc_stale_best"] += 1
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpRelocCandidates = []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if pKFi.mnId not in spAlreadyAddedKF:
                    vpRelocCandidates.append(pKFi.mnId)
                    spAlreadyAddedKF.add(pKFi.mnId)
                else:
                    C["reloc_dedup_dropped"] += 1
            else:
                C["reloc_below_retain"] += 1
        return vpRelocCandidates

    # src/KeyFrameDatabase.cc:76-217
    def DetectLoopCandidates(self, pKF_mnId, pKF_bow, connected, minScore):
        C = self.counters
        minScore = F32(minScore)
        spConnectedKeyFrames = set(int(x) for x in connected)
        lKFsSharingWords = []
        for w in pKF_bow[0]:
            for pKFi in self.mvInvertedFile.get(int(w), ()):
                if pKFi.mnLoopQuery != pKF_mnId:
                    pKFi.mnLoopWords = 0
                    if pKFi.mnId not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = pKF_mnId
                        lKFsSharingWords.append(pKFi)
                    else:
                        C["loop_connected_reset"] += 1
                pKFi.mnLoopWords += 1
        if not lKFsSharingWords:
            C["loop_nothing_shared"] += 1
            return []
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > maxCommonWords:
                maxCommonWords = pKFi.mnLoopWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        self.last_min_common = minCommonWords
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                si = F32(score(pKF_bow, pKFi.mBowVec))
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
                else:
                    C["loop_below_min_score"] += 1
            else:
                C["loop_not_scored"] += 1
        if not lScoreAndMatch:
            C["loop_no_match"] += 1
            return []
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):
                if pKF2.mnLoopQuery == pKF_mnId and pKF2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpLoopCandidates = []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if pKFi.mnId not in spAlreadyAddedKF:
                    vpLoopCandidates.append(pKFi.mnId)
                    spAlreadyAddedKF.add(pKFi.mnId)
                else:
                    C["loop_dedup_dropped"] += 1
        return vpLoopCandidates

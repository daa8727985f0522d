"""A literal Python restatement of ORB_SLAM2::KeyFrameDatabase (src/KeyFrameDatabase.cc:33-309) and DBoW2's
L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68): the expected values of the keyframe-database tests.

A real inverted file (one list of keyframes per word, add / erase / clear as the reference's), the per-keyframe query
marks (mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore), Python floats for the doubles
and numpy.float32 for every float operation (* 0.8f, the casts of the score, accScore +=, 0.75f *).  Each Detect* call
leaves a trace of what it decided in `last_trace`.

One value is pinned: the reference never initialises mRelocScore (KeyFrame.cc:35); it is 0.0f here until first scored.
mnLoopQuery / mnRelocQuery start at 0 as in the reference, so the query ids handed out by this module start at 1."""
import bisect
import itertools
import math

import numpy as np

f32 = np.float32


def l1_score(v1, v2):
    """L1Scoring::score(v1, v2), v1 / v2 dicts {word: value} (std::map: walked in ascending word order)."""
    k1, k2 = sorted(v1), sorted(v2)
    i, j = 0, 0
    score = 0.0
    while i < len(k1) and j < len(k2):
        vi, wi = v1[k1[i]], v2[k2[j]]
        if k1[i] == k2[j]:
            score += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)
            i += 1
            j += 1
        elif k1[i] < k2[j]:
            i = bisect.bisect_left(k1, k2[j])    # v1.lower_bound(v2_it->first)
        else:
            j = bisect.bisect_left(k2, k1[i])
    score = -score / 2.0
    return score


def min_common_words(max_common_words):
    """int minCommonWords = maxCommonWords*0.8f;  (:120, :235)"""
    return int(f32(max_common_words) * f32(0.8))


class KeyFrame:
    def __init__(self, mnId, bow):
        self.mnId = mnId
        self.mBowVec = dict(bow)
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore = 0, 0, f32(0)
        self.mnRelocQuery, self.mnRelocWords = 0, 0
        self.mRelocScore = f32(0)    # PINNED (uninitialised upstream)
        self.connected = []          # GetConnectedKeyFrames()
        self.best_covisibles = []    # GetBestCovisibilityKeyFrames(N) returns the first N

    def GetBestCovisibilityKeyFrames(self, N):
        return list(self.best_covisibles[:N])


class Frame:
    def __init__(self, mnId, bow):
        self.mnId = mnId
        self.mBowVec = dict(bow)


_query_ids = itertools.count(1)


def next_query_id():
    return next(_query_ids)


class KeyFrameDatabase:
    def __init__(self):
        self.mvInvertedFile = {}    # word -> list of keyframes, in add order (std::vector<list<KeyFrame*>>)
        self.last_trace = None

    def add(self, pKF):
        for w in sorted(pKF.mBowVec):
            self.mvInvertedFile.setdefault(w, []).append(pKF)

    def erase(self, pKF):
        for w in sorted(pKF.mBowVec):
            lKFs = self.mvInvertedFile.get(w, [])
            for k, x in enumerate(lKFs):
                if x is pKF:
                    del lKFs[k]
                    break

    def clear(self):
        self.mvInvertedFile = {}

    # ---- the sharing list alone, with every listed keyframe scored: what orb_kfdb_query returns ----
    def sharing(self, bow, excluded=()):
        """-> [(keyframe, common words, double score)] in lKFsSharingWords order (:86-104 with excluded =
        spConnectedKeyFrames, :207-222 without)."""
        qid = next_query_id()
        lst = []
        for w in sorted(bow):
            for pKFi in self.mvInvertedFile.get(w, []):
                if pKFi.mnLoopQuery != qid:
                    pKFi.mnLoopWords = 0
                    if not any(pKFi is c for c in excluded):
                        pKFi.mnLoopQuery = qid
                        lst.append(pKFi)
                pKFi.mnLoopWords += 1
        return [(k, k.mnLoopWords, l1_score(bow, k.mBowVec)) for k in lst]

    def DetectLoopCandidates(self, pKF, minScore):
        minScore = f32(minScore)
        tr = self.last_trace = {"sharing": [], "scored": [], "kept": [], "counted": [], "acc": [], "retain": None}
        spConnectedKeyFrames = pKF.connected
        lKFsSharingWords = []
        for w in sorted(pKF.mBowVec):
            for pKFi in self.mvInvertedFile.get(w, []):
                if pKFi.mnLoopQuery != pKF.mnId:
                    pKFi.mnLoopWords = 0
                    if not any(pKFi is c for c in spConnectedKeyFrames):
                        pKFi.mnLoopQuery = pKF.mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        tr["sharing"] = [(k.mnId, k.mnLoopWords) for k in lKFsSharingWords]
        if not lKFsSharingWords:
            return []
        lScoreAndMatch = []
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnLoopWords > maxCommonWords:
                maxCommonWords = k.mnLoopWords
        minCommonWords = min_common_words(maxCommonWords)
        tr["min_common"] = minCommonWords
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                d = l1_score(pKF.mBowVec, pKFi.mBowVec)
                si = f32(d)
                tr["scored"].append((pKFi.mnId, d))
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
                    tr["kept"].append(pKFi.mnId)
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            vpNeighs = pKFi.GetBestCovisibilityKeyFrames(10)
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in vpNeighs:
                if pKF2.mnLoopQuery == pKF.mnId and pKF2.mnLoopWords > minCommonWords:
                    tr["counted"].append((pKFi.mnId, pKF2.mnId))
                    accScore = f32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            tr["acc"].append((pKFi.mnId, float(accScore), pBestKF.mnId))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        tr["retain"] = float(minScoreToRetain)
        spAlreadyAddedKF = []
        vpLoopCandidates = []
        for acc, pKFi in lAccScoreAndMatch:
            if acc > minScoreToRetain:
                if not any(pKFi is x for x in spAlreadyAddedKF):
                    vpLoopCandidates.append(pKFi)
                    spAlreadyAddedKF.append(pKFi)
        return vpLoopCandidates

    def DetectRelocalizationCandidates(self, F):
        tr = self.last_trace = {"sharing": [], "scored": [], "kept": [], "counted": [], "acc": [], "retain": None}
        lKFsSharingWords = []
        for w in sorted(F.mBowVec):
            for pKFi in self.mvInvertedFile.get(w, []):
                if pKFi.mnRelocQuery != F.mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        tr["sharing"] = [(k.mnId, k.mnRelocWords) for k in lKFsSharingWords]
        if not lKFsSharingWords:
            return []
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnRelocWords > maxCommonWords:
                maxCommonWords = k.mnRelocWords
        minCommonWords = min_common_words(maxCommonWords)
        tr["min_common"] = minCommonWords
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                d = l1_score(F.mBowVec, pKFi.mBowVec)
                si = f32(d)
                tr["scored"].append((pKFi.mnId, d))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
                tr["kept"].append(pKFi.mnId)
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = f32(0)
        for si, pKFi in lScoreAndMatch:
            vpNeighs = pKFi.GetBestCovisibilityKeyFrames(10)
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in vpNeighs:
                if pKF2.mnRelocQuery != F.mnId:
                    continue
                tr["counted"].append((pKFi.mnId, pKF2.mnId, float(pKF2.mRelocScore)))
                accScore = f32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            tr["acc"].append((pKFi.mnId, float(accScore), pBestKF.mnId))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        tr["retain"] = float(minScoreToRetain)
        spAlreadyAddedKF = []
        vpRelocCandidates = []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if not any(pKFi is x for x in spAlreadyAddedKF):
                    vpRelocCandidates.append(pKFi)
                    spAlreadyAddedKF.append(pKFi)
        return vpRelocCandidates

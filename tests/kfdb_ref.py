"""Pure-Python restatement of ORB_SLAM2::KeyFrameDatabase (KeyFrameDatabase.cc:33-309) and of DBoW2's
L1Scoring::score, the oracle of tests/test_kfdb.py, tests/test_gpu_kfdb.py. Literal: an inverted file of lists, the
per-keyframe query / words / score fields, connected sets and neighbour lists; state persists across calls."""
import numpy as np


def l1_terms(v1, v2):
    """The per-common-word terms of L1Scoring::score(v1, v2), in ascending word id. v = (words, values)."""
    w1, x1 = v1
    w2, x2 = v2
    terms, common = [], []
    i, j, n1, n2 = 0, 0, len(w1), len(w2)
    while i < n1 and j < n2:
        if w1[i] == w2[j]:
            vi, wi = float(x1[i]), float(x2[j])
            terms.append((abs(vi - wi) - abs(vi)) - abs(wi))
            common.append(int(w1[i]))
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            i += 1  # lower_bound in DBoW2: same walk
        else:
            j += 1
    return terms, common


def l1_score(v1, v2):
    """(score as np.float32, ncommon, first common word or 0xFFFFFFFF). Python floats are doubles; one add after
    another in ascending word order; `float si = ...` narrows."""
    terms, common = l1_terms(v1, v2)
    s = 0.0
    for t in terms:
        s += t
    return np.float32(-s / 2.0), len(common), (common[0] if common else 0xFFFFFFFF)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


class KF:
    """The KeyFrame members KeyFrameDatabase reads and writes."""
    _next = 0

    def __init__(self, words, values, key=None):
        self.mnId = KF._next
        KF._next += 1
        self.key = self.mnId if key is None else key
        self.bow = (np.asarray(words, np.uint32), np.asarray(values, np.float64))
        self.mnLoopQuery = -1
        self.mnLoopWords = 0
        self.mLoopScore = np.float32(0)
        self.mnRelocQuery = -1
        self.mnRelocWords = 0
        self.mRelocScore = np.float32(0)
        self.connected = set()  # GetConnectedKeyFrames()
        self.neigh = []         # GetBestCovisibilityKeyFrames(10)


class RefDatabase:
    def __init__(self):
        self.inv = {}  # mvInvertedFile: word -> list of KF

    def add(self, kf):
        for w in kf.bow[0]:
            self.inv.setdefault(int(w), []).append(kf)

    def erase(self, kf):
        for w in kf.bow[0]:
            lst = self.inv.get(int(w), [])
            for i, k in enumerate(lst):
                if k is kf:
                    del lst[i]
                    break

    def clear(self):
        self.inv = {}

    def detect_loop_candidates(self, pKF, minScore):
        minScore = np.float32(minScore)
        sharing = []
        for w in pKF.bow[0]:
            for pKFi in self.inv.get(int(w), []):
                if pKFi.mnLoopQuery != pKF.mnId:
                    pKFi.mnLoopWords = 0
                    if pKFi not in pKF.connected:
                        pKFi.mnLoopQuery = pKF.mnId
                        sharing.append(pKFi)
                pKFi.mnLoopWords += 1
        if not sharing:
            return []
        maxCommonWords = 0
        for k in sharing:
            if k.mnLoopWords > maxCommonWords:
                maxCommonWords = k.mnLoopWords
        minCommonWords = int(np.float32(maxCommonWords) * np.float32(0.8))
        lScoreAndMatch = []
        for pKFi in sharing:
            if pKFi.mnLoopWords > minCommonWords:
                si = l1_score(pKF.bow, pKFi.bow)[0]
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return []
        lAcc = []
        bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in pKFi.neigh[:10]:
                if pKF2.mnLoopQuery == pKF.mnId and pKF2.mnLoopWords > minCommonWords:
                    accScore = np.float32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAcc.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = np.float32(np.float32(0.75) * bestAccScore)
        out = []
        for acc, k in lAcc:
            if acc > minScoreToRetain and k not in out:
                out.append(k)
        return out

    def detect_relocalization_candidates(self, F):
        sharing = []
        for w in F.bow[0]:
            for pKFi in self.inv.get(int(w), []):
                if pKFi.mnRelocQuery != F.mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    sharing.append(pKFi)
                pKFi.mnRelocWords += 1
        if not sharing:
            return []
        maxCommonWords = 0
        for k in sharing:
            if k.mnRelocWords > maxCommonWords:
                maxCommonWords = k.mnRelocWords
        minCommonWords = int(np.float32(maxCommonWords) * np.float32(0.8))
        lScoreAndMatch = []
        for pKFi in sharing:
            if pKFi.mnRelocWords > minCommonWords:
                si = l1_score(F.bow, pKFi.bow)[0]
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return []
        lAcc = []
        bestAccScore = np.float32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in pKFi.neigh[:10]:
                if pKF2.mnRelocQuery != F.mnId:
                    continue
                accScore = np.float32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAcc.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = np.float32(np.float32(0.75) * bestAccScore)
        out = []
        for acc, k in lAcc:
            if acc > minScoreToRetain and k not in out:
                out.append(k)
        return out

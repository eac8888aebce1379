"""Sequential restatement of the reference's KeyFrameDatabase (src/KeyFrameDatabase.cc): add (:39-45), erase (:47-66), clear
(:68-72), DetectNBestCandidates (:604-730), DetectRelocalizationCandidates (:733-845) and DBoW2's L1Scoring::score
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), line for line: a real list of keyframes per word, the per-keyframe members, a
numpy.float64 accumulator that is added to term by term, numpy.float32 where the reference has `float`.  The parity target of
ft_kfdb_*; it shares no code with the library."""
import bisect

import numpy as np

F32, F64 = np.float32, np.float64


class KeyFrame:
    """the members the two queries touch (KeyFrame.cc:33-34: all start at 0); `handle` = the add sequence number"""

    def __init__(self, handle, ids, values):
        self.handle = handle
        self.ids = [int(i) for i in ids]           # mBowVec: std::map<WordId, WordValue>, ascending
        self.values = [F64(v) for v in values]
        self.mnPlaceRecognitionQuery = 0
        self.mnPlaceRecognitionWords = 0
        self.mPlaceRecognitionScore = F32(0)
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = F32(0)


def l1_score(ids1, values1, ids2, values2, reverse=False):
    """L1Scoring::score(v1, v2) -> (the double it returns, the float `float si =` makes of it).  reverse=True adds the same terms
    in descending word order (the power check of the tests; never the parity target)."""
    terms = []
    i1, i2, n1, n2 = 0, 0, len(ids1), len(ids2)
    while i1 != n1 and i2 != n2:
        vi, wi = values1[i1], values2[i2]
        if ids1[i1] == ids2[i2]:
            terms.append(np.abs(vi - wi) - np.abs(vi) - np.abs(wi))
            i1 += 1
            i2 += 1
        elif ids1[i1] < ids2[i2]:
            i1 = bisect.bisect_left(ids1, ids2[i2])   # v1.lower_bound(v2_it->first)
        else:
            i2 = bisect.bisect_left(ids2, ids1[i1])
    score = F64(0)
    for t in (reversed(terms) if reverse else terms):
        score = score + t                            # score += fabs(vi - wi) - fabs(vi) - fabs(wi)
    score = -score / F64(2.0)
    return score, F32(score)


class KeyFrameDatabase:
    PLACE, RELOC = 0, 1

    def __init__(self):
        self.mvInvertedFile = {}   # word -> list of KeyFrame (the vector of lists, sparse)
        self.keyframes = {}        # handle -> KeyFrame, the live ones
        self.next_handle = 0

    def add(self, ids, values):
        pKF = KeyFrame(self.next_handle, ids, values)
        self.next_handle += 1
        for w in pKF.ids:
            self.mvInvertedFile.setdefault(w, []).append(pKF)
        self.keyframes[pKF.handle] = pKF
        return pKF.handle

    def erase(self, handle):
        pKF = self.keyframes.pop(handle)
        for w in pKF.ids:
            lKFs = self.mvInvertedFile[w]
            for k, other in enumerate(lKFs):
                if other is pKF:
                    del lKFs[k]
                    break

    def clear(self):
        self.mvInvertedFile = {}
        self.keyframes = {}

    def state(self, kind, handles):
        kfs = [self.keyframes[int(h)] for h in handles]
        if kind == self.PLACE:
            return (np.array([k.mnPlaceRecognitionQuery for k in kfs], np.int64), np.array([k.mnPlaceRecognitionWords for k in kfs], np.int32),
                    np.array([k.mPlaceRecognitionScore for k in kfs], np.float32))
        return (np.array([k.mnRelocQuery for k in kfs], np.int64), np.array([k.mnRelocWords for k in kfs], np.int32),
                np.array([k.mRelocScore for k in kfs], np.float32))

    # ---- the part of both queries that ft_kfdb_score covers: :615-666 and :741-787 ----
    def score(self, kind, query_id, ids, values, connected=()):
        ids = [int(i) for i in ids]
        values = [F64(v) for v in values]
        spConnectedKF = set(int(h) for h in connected)
        lKFsSharingWords = []
        for w in ids:
            for pKFi in self.mvInvertedFile.get(w, []):
                if kind == self.PLACE:
                    if pKFi.mnPlaceRecognitionQuery != query_id:
                        pKFi.mnPlaceRecognitionWords = 0
                        if pKFi.handle not in spConnectedKF:
                            pKFi.mnPlaceRecognitionQuery = query_id
                            lKFsSharingWords.append(pKFi)
                    pKFi.mnPlaceRecognitionWords += 1
                else:
                    if pKFi.mnRelocQuery != query_id:
                        pKFi.mnRelocWords = 0
                        pKFi.mnRelocQuery = query_id
                        lKFsSharingWords.append(pKFi)
                    pKFi.mnRelocWords += 1
        out = dict(n_sharing=len(lKFsSharingWords), max_common_words=0, min_common_words=0, handles=[], words=[], scores=[], raw_scores=[],
                   listed=[k.handle for k in lKFsSharingWords])
        if not lKFsSharingWords:
            return _arrays(out)
        words = (lambda k: k.mnPlaceRecognitionWords) if kind == self.PLACE else (lambda k: k.mnRelocWords)
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:
            if words(pKFi) > maxCommonWords:
                maxCommonWords = words(pKFi)
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))   # int minCommonWords = maxCommonWords*0.8f
        out["max_common_words"], out["min_common_words"] = maxCommonWords, minCommonWords
        for pKFi in lKFsSharingWords:
            if words(pKFi) > minCommonWords:
                raw, si = l1_score(ids, values, pKFi.ids, pKFi.values)
                if kind == self.PLACE:
                    pKFi.mPlaceRecognitionScore = si
                else:
                    pKFi.mRelocScore = si
                out["handles"].append(pKFi.handle)
                out["words"].append(words(pKFi))
                out["scores"].append(si)
                out["raw_scores"].append(raw)
        return _arrays(out)

    # ---- :671-700 / :792-821: lAccScoreAndMatch ----
    def _accumulate(self, kind, query_id, scored, neighbours):
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for h, si in zip(scored["handles"], scored["scores"]):
            bestScore = F32(si)
            accScore = bestScore
            pBestKF = int(h)
            for h2 in neighbours(int(h)):
                pKF2 = self.keyframes[int(h2)]
                stamp, stored = ((pKF2.mnPlaceRecognitionQuery, pKF2.mPlaceRecognitionScore) if kind == self.PLACE
                                 else (pKF2.mnRelocQuery, pKF2.mRelocScore))
                if stamp != query_id:
                    continue
                accScore = F32(accScore + stored)
                if stored > bestScore:
                    pBestKF = int(h2)
                    bestScore = stored
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return lAccScoreAndMatch, bestAccScore

    def select_n_best(self, query_id, scored, neighbours, maps, query_map, n_candidates, bad_maps=()):
        """:668-729 -> (vpLoopCand, vpMergeCand)"""
        if len(scored["handles"]) == 0:
            return [], []
        lAccScoreAndMatch, _ = self._accumulate(self.PLACE, query_id, scored, neighbours)
        lAccScoreAndMatch = _list_sort_descending(lAccScoreAndMatch)
        vpLoopCand, vpMergeCand, spAlreadyAddedKF = [], [], set()
        i = 0
        while i < len(lAccScoreAndMatch) and (len(vpLoopCand) < n_candidates or len(vpMergeCand) < n_candidates):
            pKFi = lAccScoreAndMatch[i][1]
            if pKFi not in spAlreadyAddedKF:
                if query_map == maps(pKFi) and len(vpLoopCand) < n_candidates:
                    vpLoopCand.append(pKFi)
                elif query_map != maps(pKFi) and len(vpMergeCand) < n_candidates and maps(pKFi) not in bad_maps:
                    vpMergeCand.append(pKFi)
                spAlreadyAddedKF.add(pKFi)
            i += 1
        return vpLoopCand, vpMergeCand

    def select_reloc(self, query_id, scored, neighbours, maps, target_map):
        """:789-844 -> vpRelocCandidates"""
        if len(scored["handles"]) == 0:
            return []
        lAccScoreAndMatch, bestAccScore = self._accumulate(self.RELOC, query_id, scored, neighbours)
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF, vpRelocCandidates = set(), []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if maps(pKFi) != target_map:
                    continue
                if pKFi not in spAlreadyAddedKF:
                    vpRelocCandidates.append(pKFi)
                    spAlreadyAddedKF.add(pKFi)
        return vpRelocCandidates


def _list_sort_descending(entries):
    """std::list::sort(compFirst) with compFirst(a, b) = a.first > b.first: a stable merge sort - entries with equal scores keep
    their order.  Written as an insertion that never passes an equal element."""
    out = []
    for e in entries:
        k = len(out)
        while k > 0 and e[0] > out[k - 1][0]:
            k -= 1
        out.insert(k, e)
    return out


def _arrays(out):
    out["handles"] = np.array(out["handles"], np.int32)
    out["words"] = np.array(out["words"], np.int32)
    out["scores"] = np.array(out["scores"], np.float32)
    out["raw_scores"] = np.array(out["raw_scores"], np.float64)
    return out

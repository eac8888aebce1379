"""Sequential restatement of ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vpMatches12) (reference
src/ORBmatcher.cc:864-1004), the matcher LoopClosing::DetectCommonRegionsFromBoW runs for the current keyframe against every
covisible keyframe of a candidate (src/LoopClosing.cc:657-668): the walk over the nodes both FeatureVectors hold, the features
of keyframe 1 in list order, every candidate of keyframe 2 in list order with the strict comparisons of :935-944, the acceptance
of :947-949, the rotation histogram, ComputeThreeMaxima and the removal.

A keyframe is a dict(fv_nodes, fv_offsets, fv_features, descriptors [n, 32], angles [n], has_point [n], n_left, n_un):
has_point[i] = GetMapPoint(i) exists and is not bad, n_left = KeyFrame::NLeft (-1 = one camera), n_un = mvKeysUn.size() (read
only when n_left != -1).  Arithmetic is float32 where the reference has floats (the ratio test is one float32 product, the
rotation bin is tests/init_search_ref.rotation_bin); ComputeThreeMaxima is the oracle's (orc_three_maxima).

The scan is written out as the reference has it - one comparison per candidate, in order -, only DescriptorDistance is taken
from a table of the node's distances computed in one numpy call.
"""
import numpy as np

from tests.init_search_ref import HISTO_LENGTH, TH_LOW, _POP8, rotation_bin, three_maxima


def _skipped_by_n_un(kf, idx):
    return kf["n_left"] != -1 and idx >= kf["n_un"]  # NLeft != -1 && idx >= mvKeysUn.size() (:899, :919)


def search_by_bow_keyframes(kf1, kf2, nn_ratio=0.9, check_orientation=True, th_low_inclusive=False):
    """-> dict(matches12 [n1] = feature of keyframe 2 whose map point vpMatches12[idx1] receives or -1, n = the return value,
    stats).  th_low_inclusive relaxes bestDist1 < TH_LOW to <= TH_LOW (the comparison of the KeyFrame, Frame overload, :426):
    for the cross-check against the oracle's search_by_bow only."""
    n1, n2 = len(kf1["descriptors"]), len(kf2["descriptors"])
    ratio = np.float32(nn_ratio)
    matches12 = np.full(n1, -1, np.int32)
    matched2 = np.zeros(n2, bool)  # vbMatched2
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    stats = dict(shared_nodes=0, node_sizes=[], eligible1=[], eligible2=[], dist_50=0, ratio_rejections=0, claims_changed_a_choice=0,
                 removed_by_histogram=0, skipped_by_n_un=0)
    nodes1 = [int(v) for v in kf1["fv_nodes"]]
    nodes2 = [int(v) for v in kf2["fv_nodes"]]
    off1, off2 = np.asarray(kf1["fv_offsets"]), np.asarray(kf2["fv_offsets"])
    i1 = i2 = 0
    while i1 < len(nodes1) and i2 < len(nodes2):  # :892
        if nodes1[i1] < nodes2[i2]:
            i1 += 1  # lower_bound: the first key not below the other side's
            continue
        if nodes1[i1] > nodes2[i2]:
            i2 += 1
            continue
        list1 = [int(v) for v in kf1["fv_features"][off1[i1]:off1[i1 + 1]]]
        list2 = [int(v) for v in kf2["fv_features"][off2[i2]:off2[i2 + 1]]]
        i1 += 1
        i2 += 1
        stats["shared_nodes"] += 1
        stats["node_sizes"].append((len(list1), len(list2)))
        stats["skipped_by_n_un"] += sum(_skipped_by_n_un(kf1, i) for i in list1) + sum(_skipped_by_n_un(kf2, i) for i in list2)
        el2 = [not _skipped_by_n_un(kf2, i) and bool(kf2["has_point"][i]) for i in list2]
        stats["eligible1"].append(sum(not _skipped_by_n_un(kf1, i) and bool(kf1["has_point"][i]) for i in list1))
        stats["eligible2"].append(sum(el2))
        if not list1 or not list2:
            continue
        # DescriptorDistance of every pair of the node
        dist_tab = _POP8[np.bitwise_xor(kf1["descriptors"][list1][:, None, :], kf2["descriptors"][list2][None, :, :])].sum(axis=2)
        for p1, idx1 in enumerate(list1):  # :896
            if _skipped_by_n_un(kf1, idx1):
                continue
            if not kf1["has_point"][idx1]:  # !pMP1 || pMP1->isBad() (:903-907)
                continue
            best_dist1, best_idx2, best_dist2 = 256, -1, 256
            blind_dist, blind_idx = 256, -1  # the same scan without vbMatched2: what the feature would take alone
            for p2, idx2 in enumerate(list2):  # :915
                if not el2[p2]:  # :919, !pMP2, isBad() (:925-929)
                    continue
                dist = int(dist_tab[p1, p2])
                if dist < blind_dist:
                    blind_dist, blind_idx = dist, idx2
                if matched2[idx2]:
                    continue
                if dist < best_dist1:
                    best_dist2 = best_dist1
                    best_dist1 = dist
                    best_idx2 = idx2
                elif dist < best_dist2:
                    best_dist2 = dist
            if blind_idx >= 0 and matched2[blind_idx]:
                stats["claims_changed_a_choice"] += 1
            if best_dist1 == TH_LOW:
                stats["dist_50"] += 1
            if best_dist1 < TH_LOW or (th_low_inclusive and best_dist1 == TH_LOW):  # :947
                if np.float32(best_dist1) < ratio * np.float32(best_dist2):  # :949
                    matches12[idx1] = best_idx2
                    matched2[best_idx2] = True
                    if check_orientation:
                        b = rotation_bin(kf1["angles"][idx1], kf2["angles"][best_idx2])
                        assert 0 <= b < HISTO_LENGTH
                        rot_hist[b].append(idx1)
                    nmatches += 1
                else:
                    stats["ratio_rejections"] += 1
    if check_orientation:  # :983-1001
        keep = three_maxima([len(b) for b in rot_hist])
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for idx1 in rot_hist[b]:
                matches12[idx1] = -1
                nmatches -= 1
                stats["removed_by_histogram"] += 1
    return dict(matches12=matches12, n=nmatches, stats=stats)

"""ORBmatcher::SearchForInitialization restated in Python, statement by statement (reference src/ORBmatcher.cc:747-862).

The checker of ft_search_for_initialization / ft_tracked_frame_search_for_initialization.  What it does not state itself is
taken from the oracle, where existing tests pin it: the candidates of a window and their order (oracle.binding.features_in_area
= Frame::GetFeaturesInArea) and ComputeThreeMaxima (orc_three_maxima); DescriptorDistance is the popcount of the XOR
(equal to oracle.binding.descriptor_distance, test_init_search_cpu.py checks that).  rot, factor and the ratio test are float32
as in the reference.  Besides the function's outputs it reports what happened on the way, so that a test can assert that its
inputs exercise the sequential part at all.
"""
import ctypes as C
import math

import numpy as np

from oracle import binding as ob

TH_LOW = 50
HISTO_LENGTH = 30
INT_MAX = 2147483647

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distances(d1: np.ndarray, d2: np.ndarray) -> np.ndarray:
    """DescriptorDistance of one 32-byte descriptor against rows of descriptors"""
    return _POP8[np.bitwise_xor(d2, d1[None, :])].sum(axis=1)


def three_maxima(sizes):
    h = np.ascontiguousarray(sizes, np.int32)
    i1, i2, i3 = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    ob.lib().orc_three_maxima(h.ctypes.data_as(C.c_void_p), len(h), C.byref(i1), C.byref(i2), C.byref(i3))
    return i1.value, i2.value, i3.value


def rotation_bin(angle1, angle2) -> int:
    """:817-822 - float arithmetic, round() = half away from zero (not cvRound)"""
    rot = np.float32(angle1) - np.float32(angle2)
    if rot < 0.0:
        rot = np.float32(rot + np.float32(360.0))
    v = float(np.float32(rot * (np.float32(1.0) / np.float32(HISTO_LENGTH))))
    b = int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)
    return 0 if b == HISTO_LENGTH else b


def search_for_initialization(keys1, desc1, F2: "ob.FrameView", prev_matched, window_size=100, nn_ratio=0.9,
                              check_orientation=True):
    """keys1 / desc1: F1.mvKeysUn (structured, .octave .angle) and F1.mDescriptors; F2: an oracle FrameView (mono);
    prev_matched: (N1, 2) float32, NOT modified.  -> dict(matches12, prev_matched, n, matched_distance, stats)."""
    N1, N2 = len(keys1), F2.N
    keys2, desc2 = F2.keys, F2.descriptors
    prev = np.array(prev_matched, np.float32).reshape(N1, 2).copy()
    ratio = np.float32(nn_ratio)
    nmatches = 0
    m12 = np.full(N1, -1, np.int32)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    matched_distance = np.full(N2, INT_MAX, np.int64)
    m21 = np.full(N2, -1, np.int32)
    st = dict(evictions=0, skipped=0, accepted=0, ratio_rejected=0, removed_by_histogram=0, evicted_in_kept_bin=0,
              evicted_changes_bins=False, candidates=0, level0=0)
    evicted = set()
    for i1 in range(N1):
        if keys1["octave"][i1] > 0:
            continue
        st["level0"] += 1
        idx2 = ob.features_in_area(F2, float(prev[i1, 0]), float(prev[i1, 1]), float(window_size), 0, 0)
        if len(idx2) == 0:
            continue
        st["candidates"] += len(idx2)
        dists = distances(desc1[i1], desc2[idx2])
        best, best2, best_idx = INT_MAX, INT_MAX, -1
        for i2, dist in zip(idx2.tolist(), dists.tolist()):
            if matched_distance[i2] <= dist:
                st["skipped"] += 1
                continue
            if dist < best:
                best2, best, best_idx = best, dist, i2
            elif dist < best2:
                best2 = dist
        if best <= TH_LOW:
            if np.float32(best) < np.float32(np.float32(best2) * ratio):
                if m21[best_idx] >= 0:
                    m12[m21[best_idx]] = -1
                    evicted.add(int(m21[best_idx]))
                    nmatches -= 1
                    st["evictions"] += 1
                m12[i1] = best_idx
                m21[best_idx] = i1
                matched_distance[best_idx] = best
                nmatches += 1
                st["accepted"] += 1
                if check_orientation:
                    b = rotation_bin(keys1["angle"][i1], keys2["angle"][best_idx])
                    assert 0 <= b < HISTO_LENGTH
                    rot_hist[b].append(i1)
            else:
                st["ratio_rejected"] += 1
    if check_orientation:
        sizes = [len(b) for b in rot_hist]
        keep = three_maxima(sizes)
        live = [sum(1 for i in b if i not in evicted) for b in rot_hist]
        st["evicted_changes_bins"] = set(three_maxima(live)) != set(keep)
        for i in range(HISTO_LENGTH):
            if i in keep:
                st["evicted_in_kept_bin"] += sum(1 for j in rot_hist[i] if j in evicted)
                continue
            for j in rot_hist[i]:
                if m12[j] >= 0:
                    m12[j] = -1
                    nmatches -= 1
                    st["removed_by_histogram"] += 1
    for i1 in range(N1):
        if m12[i1] >= 0:
            prev[i1, 0] = keys2["x"][m12[i1]]
            prev[i1, 1] = keys2["y"][m12[i1]]
    return dict(matches12=m12, prev_matched=prev, n=nmatches, matched_distance=matched_distance.astype(np.int32), stats=st)

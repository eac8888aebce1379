"""ORBmatcher::SearchForInitialization (reference src/ORBmatcher.cc:747-862): the Python restatement the GPU tests compare
against (tests/init_search_ref.py) on hand-built cases whose expected results are written out here from the reference text,
and the C ABI of the two entry points without a device."""
import ctypes as C

import numpy as np

from fasttrack_amd import _capi
from oracle import binding as ob
from tests import init_search_ref as ref

KP = ob.KP_DTYPE
W, H = 640, 480   # image bounds (0, 0, 640, 480): grid cells of 10 x 10 pixels
SF, _ = ob.scale_factors(1.2, 8)


def _keys(xy, octave=None, angle=None):
    k = np.zeros(len(xy), KP)
    k["x"], k["y"] = [p[0] for p in xy], [p[1] for p in xy]
    k["size"] = 31
    k["octave"] = 0 if octave is None else octave
    k["angle"] = 0 if angle is None else angle
    return k


def _flip(d, bits):
    d = d.copy()
    for b in bits:
        d[b // 8] ^= 1 << (b % 8)
    return d


def _frame(keys, desc):
    return ob.FrameView(keys, np.asarray(desc, np.uint8).reshape(len(keys), 32), SF, (0, 0, W, H))


BASE = np.random.default_rng(7).integers(0, 256, (64, 32), dtype=np.uint8)  # pairwise about 128 bits apart


def test_descriptor_distance_is_the_oracles():
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 256, (50, 32), dtype=np.uint8), rng.integers(0, 256, (50, 32), dtype=np.uint8)
    for i in range(50):
        assert ref.distances(a[i], b[i:i + 1])[0] == ob.descriptor_distance(a[i], b[i])
    assert ref.distances(a[0], _flip(a[0], range(7))[None])[0] == 7


def test_a_later_strictly_closer_keypoint_evicts_the_owner():
    """(a) :805-813: the loser ends at -1, nmatches is net +0 for the second keypoint; (d) a lone candidate passes the ratio
    test against INT_MAX"""
    F2 = _frame(_keys([(100.25, 100.5)]), [BASE[0]])
    k1 = _keys([(100, 100), (101, 99)])
    d1 = np.stack([_flip(BASE[0], range(10)), _flip(BASE[0], range(20, 23))])
    prev = np.array([[100, 100], [101, 99]], np.float32)
    one = ref.search_for_initialization(k1[:1], d1[:1], F2, prev[:1])
    assert one["n"] == 1 and one["matches12"].tolist() == [0] and one["matched_distance"].tolist() == [10]
    r = ref.search_for_initialization(k1, d1, F2, prev)
    assert r["n"] == 1 and r["matches12"].tolist() == [-1, 0]
    assert r["matched_distance"].tolist() == [3] and r["stats"]["evictions"] == 1
    # (i) vbPrevMatched: the final match moves to F2's keypoint, the evicted one keeps its position
    assert r["prev_matched"].tolist() == [[100, 100], [100.25, 100.5]]


def test_equal_distance_does_not_evict():
    """(b) :786 `vMatchedDistance[i2] <= dist` skips the candidate"""
    F2 = _frame(_keys([(100, 100)]), [BASE[0]])
    k1 = _keys([(100, 100), (101, 99)])
    d1 = np.stack([_flip(BASE[0], range(10)), _flip(BASE[0], range(20, 30))])
    r = ref.search_for_initialization(k1, d1, F2, np.array([[100, 100], [101, 99]], np.float32))
    assert r["n"] == 1 and r["matches12"].tolist() == [0, -1]
    assert r["stats"]["skipped"] == 1 and r["stats"]["evictions"] == 0


def test_first_of_equal_distances_wins_and_fails_the_ratio_test():
    """(c) strict < at :789: the first candidate in GetFeaturesInArea order (cell column first) is the best, the other the
    second best at the same distance - rejected at ratio 0.9; a ratio above 1 shows who the best was: keypoint 1, in the
    earlier cell column, not keypoint 0 with the smaller index"""
    F2 = _frame(_keys([(120, 100), (100, 100)]), [_flip(BASE[0], range(5)), _flip(BASE[0], range(40, 45))])
    k1, d1, prev = _keys([(105, 100)]), BASE[:1], np.array([[105, 100]], np.float32)
    assert ob.features_in_area(F2, 105.0, 100.0, 100.0, 0, 0).tolist() == [1, 0]
    r = ref.search_for_initialization(k1, d1, F2, prev, nn_ratio=0.9)
    assert r["n"] == 0 and r["matches12"].tolist() == [-1] and r["stats"]["ratio_rejected"] == 1
    r = ref.search_for_initialization(k1, d1, F2, prev, nn_ratio=1.5)
    assert r["n"] == 1 and r["matches12"].tolist() == [1]


def test_th_low_is_inclusive():
    """(e) :801 bestDist <= TH_LOW (50)"""
    F2 = _frame(_keys([(100, 100), (300, 300)]), [_flip(BASE[0], range(50)), _flip(BASE[1], range(51))])
    r = ref.search_for_initialization(_keys([(100, 100), (300, 300)]), BASE[:2], F2, np.array([[100, 100], [300, 300]], np.float32))
    assert r["matches12"].tolist() == [0, -1] and r["n"] == 1


def test_only_level_zero_on_both_sides():
    """(f) :764 octave > 0 of F1 is skipped; GetFeaturesInArea(.., 0, 0) never returns a level-1 keypoint of F2"""
    F2 = _frame(_keys([(100, 100), (102, 100)], octave=[1, 0]), [BASE[0], _flip(BASE[0], range(20))])
    k1 = _keys([(100, 100), (100, 100)], octave=[1, 0])
    r = ref.search_for_initialization(k1, np.stack([BASE[0], BASE[0]]), F2, np.array([[100, 100], [100, 100]], np.float32))
    assert r["matches12"].tolist() == [-1, 1] and r["n"] == 1 and r["matched_distance"].tolist() == [ref.INT_MAX, 20]


def _bins_case(spec, window=15):
    """spec: (angle1, angle2, bits flipped, target) per keypoint of F1, in order; target t sits at (40 + 40 t, 100)"""
    nt = 1 + max(s[3] for s in spec)
    a2 = np.zeros(nt, np.float32)
    for a1_, a2_, _, t in spec:
        a2[t] = a2_
    F2 = _frame(_keys([(40 + 40 * t + 0.5, 100.25) for t in range(nt)], angle=a2), BASE[:nt])
    k1 = _keys([(40 + 40 * s[3], 100) for s in spec], angle=[s[0] for s in spec])
    d1 = np.stack([_flip(BASE[s[3]], range(s[2])) for s in spec])
    prev = np.array([(40 + 40 * s[3], 100) for s in spec], np.float32)
    return ref.search_for_initialization(k1, d1, F2, prev, window_size=window), prev


def test_an_evicted_keypoint_still_counts_in_its_rotation_bin():
    """(g) :824 pushes i1 into its bin, the eviction at :807 does not take it out: ComputeThreeMaxima sees bins 0 .. 3 with
    4, 4, 3 (one live, two evicted) and 2 entries and keeps 0, 1, 2 - the two matches of bin 3 go (9 matches).  Counting live
    entries only (4, 4, 1, 2) would keep bin 3 and drop bin 2 (10 matches)."""
    spec = [(60, 0, 10, 0), (60, 0, 10, 1),           # evicted later, stay in bin 2
            (0, 0, 3, 0), (0, 0, 3, 1), (0, 0, 0, 2), (0, 0, 0, 3),   # bin 0: two of them evict
            (30, 0, 0, 4), (30, 0, 0, 5), (30, 0, 0, 6), (30, 0, 0, 7),   # bin 1
            (60, 0, 0, 8),                             # bin 2, live
            (90, 0, 0, 9), (90, 0, 0, 10)]            # bin 3
    r, prev = _bins_case(spec)
    assert r["matches12"].tolist() == [-1, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, -1, -1]
    assert r["n"] == 9
    st = r["stats"]
    assert st["evictions"] == 2 and st["removed_by_histogram"] == 2 and st["evicted_in_kept_bin"] == 2 and st["evicted_changes_bins"]
    # (i) vbPrevMatched moves for the nine final matches only
    moved = (r["prev_matched"] != prev).any(axis=1)
    assert moved.tolist() == [m >= 0 for m in r["matches12"].tolist()]
    for i1, i2 in enumerate(r["matches12"].tolist()):
        if i2 >= 0:
            assert r["prev_matched"][i1].tolist() == [40 + 40 * i2 + 0.5, 100.25]
    # vMatchedDistance keeps the distance of a match the histogram removed
    assert r["matched_distance"].tolist() == [3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]


def test_rotation_bins_follow_the_reference_arithmetic():
    """(h) factor = 1.0f / HISTO_LENGTH: a rotation just below 0 wraps to just below 360 and lands in bin 12, a small positive
    one in bin 0; round() goes half away from zero where cvRound would go to even: 15 * factor is exactly 0.5f -> bin 1,
    135 -> 4.5f -> bin 5, 255 -> 8.5f -> bin 9"""
    assert ref.rotation_bin(0.0, 0.5) == 12 and ref.rotation_bin(0.5, 0.0) == 0 and ref.rotation_bin(10.0, 10.0) == 0
    assert ref.rotation_bin(15.0, 0.0) == 1 and ref.rotation_bin(135.0, 0.0) == 5 and ref.rotation_bin(255.0, 0.0) == 9
    assert ref.rotation_bin(359.99, 0.0) == 12
    # bins 12 (three at -0.5), 0 (two at +0.5), 2 (two), 3 (one): bin 3 goes; with -0.5 in bin 0 all three bins would stay
    spec = [(0, 0.5, 0, 0), (0, 0.5, 0, 1), (0, 0.5, 0, 2), (0.5, 0, 0, 3), (0.5, 0, 0, 4), (60, 0, 0, 5), (60, 0, 0, 6), (90, 0, 0, 7)]
    r, _ = _bins_case(spec)
    assert r["matches12"].tolist() == [0, 1, 2, 3, 4, 5, 6, -1] and r["n"] == 7
    # bins 0 (four), 1 (three at 15 degrees), 2 (two), 3 (two): bin 3 goes; cvRound would put 15 degrees into bin 0 and
    # keep bins 0, 2, 3
    spec = [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 0, 2), (0, 0, 0, 3), (15, 0, 0, 4), (15, 0, 0, 5), (15, 0, 0, 6),
            (60, 0, 0, 7), (60, 0, 0, 8), (90, 0, 0, 9), (90, 0, 0, 10)]
    r, _ = _bins_case(spec)
    assert r["matches12"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, -1, -1] and r["n"] == 9


def test_without_orientation_check_nothing_is_removed():
    spec = [(0, 0, 0, 0), (0, 0, 0, 1), (90, 0, 0, 2), (180, 0, 0, 3), (270, 0, 0, 4)]
    nt = 5
    F2 = _frame(_keys([(40 + 40 * t, 100) for t in range(nt)]), BASE[:nt])
    k1 = _keys([(40 + 40 * s[3], 100) for s in spec], angle=[s[0] for s in spec])
    prev = np.array([(40 + 40 * s[3], 100) for s in spec], np.float32)
    assert ref.search_for_initialization(k1, BASE[:nt], F2, prev, 15, 0.9, True)["n"] == 4
    assert ref.search_for_initialization(k1, BASE[:nt], F2, prev, 15, 0.9, False)["n"] == 5


def test_entry_points_are_declared_exported_and_reject_null_arguments_without_a_device():
    names = _capi.declared_symbols()
    L = _capi.lib()
    for name in ("ft_search_for_initialization", "ft_tracked_frame_search_for_initialization"):
        assert name in names
        assert hasattr(L, name)
    n = C.c_int(7)
    m12 = np.zeros(4, np.int32)
    prev = np.zeros((4, 2), np.float32)
    F = _capi.FrameView()
    F.N, F.Nleft = 0, -1
    args = (C.byref(F), C.byref(F), _capi.ptr(prev), 100, 0.9, 1, _capi.ptr(m12), C.byref(n), None)
    assert L.ft_search_for_initialization(None, *args) == _capi.FT_ERR_INVALID
    assert b"null" in L.ft_last_error()
    assert L.ft_search_for_initialization(None, None, None, None, 100, 0.9, 1, None, None, None) == _capi.FT_ERR_INVALID
    assert L.ft_tracked_frame_search_for_initialization(None, None, _capi.ptr(prev), 100, 0.9, 1, _capi.ptr(m12),
                                                        C.byref(n)) == _capi.FT_ERR_INVALID
    assert n.value == 7

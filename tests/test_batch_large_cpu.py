"""The large-frame cases of test_gpu_batch_large.py, checked without a GPU: the thresholds they straddle are still the library's,
scenarios.padded_in_front builds what it says, and - on the oracle alone - the cases are not vacuous."""
import re

import numpy as np
import pytest

from tests import batch_large_cases as bc
from tests import scenarios as sc


def test_thresholds_of_the_last_writer_tables_are_the_ones_the_cases_straddle():
    """k_resolve_batch keeps its table in LDS up to 12 288 keypoints, k_replay_batch up to 15 360.  Whoever moves a threshold in
    tracked_batch.cpp moves RESOLVE_LDS_MAX / REPLAY_LDS_MAX (tests/batch_large_cases.py) with it: the regimes sit on its two sides."""
    src = open(bc.TRACKED_BATCH_CPP).read()
    assert re.search(r"c\.shInts\s*<=\s*%d\b" % bc.RESOLVE_LDS_MAX, src), "callResolve: `c.shInts <= 12288` is gone"
    assert re.search(r"maxN\s*<=\s*%d\b" % bc.REPLAY_LDS_MAX, src), "replayShared: `maxN <= 15360` is gone"
    assert (bc.RESOLVE_LDS_MAX, bc.REPLAY_LDS_MAX) == (12288, 15360)
    assert bc.REGIMES == (12288, 12289, 15360, 15361)


@pytest.mark.parametrize("n_total", bc.REGIMES + (0, 1, 2))
def test_padded_in_front(n_total):
    """(0, 1, 2: that many padding keypoints - none, the right camera alone, one per camera)"""
    fr = bc.base_frame()
    nl, nr = len(fr["kL"]), len(fr["kR"])
    if n_total < 3:
        n_total += nl + nr
    a = sc.padded_in_front(fr, n_total, 5, bc.W, bc.H)
    padL, padR = a["padL"], a["padR"]
    # the counts: exactly n_total, half of the padding per camera
    assert len(a["kL"]) + len(a["kR"]) == n_total and len(a["dL"]) == len(a["kL"]) and len(a["dR"]) == len(a["kR"])
    assert padL + padR == n_total - nl - nr and 0 <= padR - padL <= 1
    assert len(a["l2r"]) == len(a["kL"]) and len(a["r2l"]) == len(a["kR"])
    # the real keypoints unchanged, in order, last
    assert np.array_equal(a["kL"][padL:], fr["kL"]) and np.array_equal(a["kR"][padR:], fr["kR"])
    assert np.array_equal(a["dL"][padL:], fr["dL"]) and np.array_equal(a["dR"][padR:], fr["dR"])
    # the padding: inside the 20 px border, octaves 0 .. 7, angles in [0, 360), size 31, no match
    for keys, n in ((a["kL"], padL), (a["kR"], padR)):
        k = keys[:n]
        assert np.all((k["x"] >= 20) & (k["x"] <= bc.W - 20) & (k["y"] >= 20) & (k["y"] <= bc.H - 20))
        assert np.all((k["octave"] >= 0) & (k["octave"] <= 7)) and np.all((k["angle"] >= 0) & (k["angle"] < 360)) and np.all(k["size"] == 31)
    if padL > 100:
        assert len(np.unique(a["kL"][:padL]["octave"])) == 8 and len(np.unique(a["dL"][:padL], axis=0)) == padL
    assert np.all(a["l2r"][:padL] == -1) and np.all(a["r2l"][:padR] == -1)
    # the match tables: the base frame's, shifted by the other camera's padding - and consistent with each other as the base's are
    assert np.array_equal(a["l2r"][padL:], np.where(fr["l2r"] >= 0, fr["l2r"] + padR, -1))
    assert np.array_equal(a["r2l"][padR:], np.where(fr["r2l"] >= 0, fr["r2l"] + padL, -1))
    assert (a["l2r"] >= 0).sum() == (fr["l2r"] >= 0).sum() > 20
    for j in np.flatnonzero(a["r2l"] >= 0):
        assert j >= padR and a["r2l"][j] >= padL and a["l2r"][a["r2l"][j]] == j
    for i in np.flatnonzero(a["l2r"] >= 0):
        j = a["l2r"][i]
        assert i >= padL and j >= padR and a["r2l"][j] >= 0 and a["l2r"][a["r2l"][j]] == j
    # one seeded generator: the same arrays again, other ones under another seed
    b = sc.padded_in_front(fr, n_total, 5, bc.W, bc.H)
    assert all(np.array_equal(a[k], b[k]) for k in ("kL", "kR", "dL", "dR", "l2r", "r2l"))
    if padL:
        assert not np.array_equal(sc.padded_in_front(fr, n_total, 6, bc.W, bc.H)["kL"], a["kL"])


def test_the_batch_of_a_regime():
    """three frames - padded to the regime's size, whole, cut to (300, 300) - and in the largest regime 30 % of the padded frame's
    keypoints held before the call, with Observations() 0, 1 and 2"""
    for n_total in bc.REGIMES:
        frames = bc.regime_case(n_total, "alternate")
        sizes = [len(f["a"]["kL"]) + len(f["a"]["kR"]) for f in frames]
        assert sizes[0] == n_total and 3800 < sizes[1] < 4100 and sizes[2] == 600
        assert ("holder" in frames[0]["a"]) == (n_total == 15361)
    h = bc.frame_arrays("padded", 15361)["holder"]
    assert len(h) == 15361 and 0.27 < (h >= 0).mean() < 0.33 and all((h == v).sum() > 1000 for v in (0, 1, 2))
    assert (h[-bc.HIGH:] > 0).sum() > 100   # real right-camera keypoints among the held ones


def test_the_hot_copies_sit_where_the_chunks_hand_over():
    """40 hot points once per 64-point chunk at positions 64 c + 3 .. 64 c + 42, Observations() per chunk as the pattern says"""
    for pattern, per_chunk in bc.PATTERNS.items():
        last, _, pts, _, _ = bc.frame_inputs("padded", pattern)
        assert len(last["valid"]) == len(pts["skip"]) == bc.POINTS == 320 and np.all(last["valid"] == 1)
        for c in range(bc.CHUNKS):
            s = slice(64 * c + 3, 64 * c + 43)
            for k in ("world_pos", "descriptors", "octave"):
                assert np.array_equal(last[k][s], last[k][3:43]), (pattern, c, k)
            for k in ("world_pos", "descriptors", "normal", "max_distance"):
                assert np.array_equal(pts[k][s], pts[k][3:43]), (pattern, c, k)
            assert np.all(last["observations"][s] == per_chunk[c]) and np.all(pts["observations"][s] == per_chunk[c])
            assert np.all(pts["skip"][s] == 0)
        assert len(np.unique(last["world_pos"], axis=0)) == 160 and len(np.unique(pts["world_pos"], axis=0)) == 160


@pytest.mark.parametrize("pattern", ["plain"] + list(bc.PATTERNS))
@pytest.mark.parametrize("n_total", bc.REGIMES)
def test_cases_are_not_vacuous_on_the_oracle(n_total, pattern):
    """What the GPU tests compare must contain what they are about (th 15, the padded frame): enough matches, matches the rotation
    histogram removes, assignments on the frame's highest keypoint indices (the real right-camera keypoints: the far end of the
    last-writer tables), points whose result depends on the chunks in front of theirs, right-camera assignments of the
    local-map search - and no candidate list beyond the cache, so that k_resolve_batch resolves the frame."""
    c = bc.conditions(n_total, pattern)
    print(n_total, pattern, c)
    assert c["last_matches"] >= 80
    assert c["removed"] >= 20
    assert c["high"] >= 15
    if pattern != "plain":   # (no copies: hand-over happens by chance only)
        assert c["chunk_dependent"] >= 50
    assert c["local_matches"] >= 120
    assert c["local_right"] >= 15
    assert c["longest_local_list"] <= bc.CACHE_CAP
    for fr in bc.regime_case(n_total, pattern)[1:]:   # the small frames beside it find something as well
        assert fr["oracle"][0]["n"] >= 30 and fr["oracle"][2]["n"] >= 30, fr["which"]

"""The two restatements of ORBmatcher::SearchByProjection(pKF, Scw, ...) (tests/sim3_search_ref.py) against each other and against
the hand-built expectations of tests/sim3_cases.py, and what the random cases of the GPU tests exercise.  No GPU."""
import numpy as np
import pytest

from tests import fuse_ref as fref
from tests import sim3_cases as s3
from tests import sim3_search_ref as ref

FIELDS = ("matched", "point_keypoint", "stage")


def agree(tag, a, b):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (tag, f, np.nonzero(a[f] != b[f])[0][:5].tolist())
    assert a["n_matches"] == b["n_matches"], tag


def test_threshold_is_the_float_comparison():
    assert ref.threshold(1.5) == 75 and ref.threshold(1.0) == 50 and ref.threshold(0.0) == 0
    assert ref.threshold(0.3) == 15                     # 50 * 0.3f = 15.000001
    assert ref.threshold(0.0199999) == 0 and ref.threshold(5.1) == 255
    assert ref.threshold(5.12) is None and ref.threshold(-0.01) is None and ref.threshold(float("nan")) is None


@pytest.mark.parametrize("name", sorted(s3.hand_cases()))
def test_hand_case(name):
    case = s3.hand_cases()[name]
    for hand in (False, True):                          # (the hand-built geometry is the same to an ulp in both forms)
        a, b = s3.run_hand_case(case, ref.search, hand), s3.run_hand_case(case, ref.search_compacted, hand)
        agree(name, a, b)
        for f in FIELDS:
            assert a[f].tolist() == case["expect"][f], (name, hand, f, a[f].tolist())
        assert a["n_matches"] == case["expect"]["n_matches"]
    if name == "past_the_top_record":
        assert b["stats"]["past_top"] == 2


@pytest.mark.parametrize("n", [5, 70])
def test_crowded_cell(n):
    case = s3.crowd_case(n)
    a, b = s3.run_hand_case(case, ref.search), s3.run_hand_case(case, ref.search_compacted)
    agree(f"crowd {n}", a, b)
    assert a["n_matches"] == n and sorted(a["point_keypoint"].tolist()) == list(range(n)) and b["stats"]["past_top"] == n - ref.TOP


def test_the_overloads_differ_on_a_window_edge():
    case, seen_by_hand = s3.overload_case()
    a, b = s3.run_hand_case(case, ref.search, False), s3.run_hand_case(case, ref.search, True)
    agree("form A", a, s3.run_hand_case(case, ref.search_compacted, False))
    agree("form B", b, s3.run_hand_case(case, ref.search_compacted, True))
    sees, blind = (b, a) if seen_by_hand else (a, b)
    assert sees["matched"].tolist() == [0] and sees["stage"].tolist() == [ref.WROTE] and sees["n_matches"] == 1
    assert blind["matched"].tolist() == [-1] and blind["stage"].tolist() == [ref.EMPTY] and blind["n_matches"] == 0


@pytest.mark.parametrize("name,th,ratio,hand", s3.USED)
def test_random_case_formulations_agree_and_exercise_the_loop(name, th, ratio, hand):
    case = s3.random_case(name)
    r = s3.expected(case, th, ratio, hand)
    oF, _ = case["view"](device=False)
    c = ref.search_compacted(oF, case["points"], case["Tcw"], case["Ow"], case["log_sf"], th, ratio, case["matched"], case["valid"], hand)
    print("sim3 non-vacuity:", name, th, ratio, hand, "n", r["n_matches"], r["stats"], c["stats"])
    agree(name, r, c)
    assert c["stats"]["walk"] == r["stats"]["walk"]
    s3.check_non_vacuous(name, case, r)
    # nothing outside the left camera and nothing held on entry is touched; what was written is what point_keypoint says
    held = case["matched"] != -1
    assert np.array_equal(r["matched"][held], case["matched"][held]) and (r["matched"][case["nleft"]:] == case["matched"][case["nleft"]:]).all()
    wrote = np.nonzero(r["point_keypoint"] >= 0)[0]
    assert np.array_equal(r["matched"][r["point_keypoint"][wrote]], wrote) and len(wrote) == r["n_matches"] == (r["stage"] == ref.WROTE).sum()


def test_the_chain_of_the_second_job_sees_the_first_jobs_writes():
    """LoopClosing.cc:755 -> :777: the second call's vpMatched is what the first left"""
    case = s3.random_case(s3.RANDOM[0])
    first = s3.expected(case, 8, 1.5, True)
    second = s3.expected(case, 5, 1.0, False, matched=first["matched"], tag="chained")
    alone = s3.expected(case, 5, 1.0, False)
    assert (first["matched"] != case["matched"]).sum() == first["n_matches"] >= 100
    assert not np.array_equal(second["point_keypoint"], alone["point_keypoint"])
    assert fref.SEARCHED == ref.WROTE and fref.EMPTY == ref.EMPTY

"""The restatement of ORBmatcher::SearchByBoW(KeyFrame, KeyFrame) (tests/bow_kf_ref.py) against what is known without a GPU: the
oracle's SearchByBoW(KeyFrame, Frame) where the two functions coincide, the hand-built cases, and the committed scenarios'
coverage of every order-dependent event.  No GPU."""
import functools

import numpy as np
import pytest

from oracle import binding as ob
from tests import bow_kf_cases as bc
from tests import bow_kf_ref as br


@functools.lru_cache(maxsize=None)
def _pair_runs(args, ori):
    """-> (the oracle's result turned around, its count, the relaxed restatement, the strict restatement)"""
    S, kf1, kf2 = bc.oracle_pair(*args)
    o = ob.search_by_bow(S["kf"], S["has_point"], S["f"], -1, 0.7, ori)
    inv = np.full(len(kf1["descriptors"]), -1, np.int32)
    idx = np.nonzero(o["matches"] >= 0)[0]
    inv[o["matches"][idx]] = idx
    assert len(set(o["matches"][idx].tolist())) == len(idx)  # a keyframe feature is matched once: the inverse exists
    return (inv, o["n"], br.search_by_bow_keyframes(kf1, kf2, 0.7, ori, th_low_inclusive=True),
            br.search_by_bow_keyframes(kf1, kf2, 0.7, ori))


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("args", bc.ORACLE_PAIRS)
def test_relaxed_restatement_is_the_inverse_of_the_oracle(args, ori):
    """one camera, every keyframe-2 feature with a point, <= TH_LOW: the two overloads walk the same nodes in the same order"""
    inv, n, relaxed, _ = _pair_runs(args, ori)
    assert np.array_equal(relaxed["matches12"], inv) and relaxed["n"] == n and n > 15


def test_the_strict_threshold_is_visible():
    """bestDist1 < TH_LOW rejects the 50 the other overload accepts: on (64, 65, 1, 3) 22 matches against the oracle's 23, and 18
    against 20 with the orientation check"""
    assert _pair_runs((64, 65, 1, 3), False)[3]["n"] == 22 and _pair_runs((64, 65, 1, 3), False)[1] == 23
    assert _pair_runs((64, 65, 1, 3), True)[3]["n"] == 18 and _pair_runs((64, 65, 1, 3), True)[1] == 20
    differing = [(a, o) for a in bc.ORACLE_PAIRS for o in (True, False)
                 if not np.array_equal(_pair_runs(a, o)[3]["matches12"], _pair_runs(a, o)[2]["matches12"])]
    assert differing
    for a, o in differing:
        assert _pair_runs(a, o)[3]["stats"]["dist_50"] > 0


@pytest.mark.parametrize("case", bc.hand_built() + bc.rotation_cases(), ids=lambda c: c["name"])
def test_hand_built_cases(case):
    for k, nb in enumerate(case["neighbours"]):
        r = br.search_by_bow_keyframes(case["kf1"], nb, case["nn_ratio"], case["check_orientation"])
        assert np.array_equal(r["matches12"], case["matches12"][k]) and r["n"] == case["n"][k], (k, r["matches12"], r["n"])


@pytest.mark.parametrize("i", range(len(bc.MAIN)))
def test_main_scenarios_are_not_vacuous(i):
    S = bc.main_scenario(i)
    two = bc.MAIN[i][1].get("two_cam", False)
    tot = dict(dist_50=0, ratio_rejections=0, claims_changed_a_choice=0, removed_by_histogram=0, skipped_by_n_un=0)
    for nb in S["neighbours"]:
        r = br.search_by_bow_keyframes(S["kf1"], nb, 0.9, True)
        assert r["stats"]["shared_nodes"] == 0 or r["n"] >= 20
        assert (nb["n_left"] != -1) == two
        for k in tot:
            tot[k] += r["stats"][k]
    assert all(tot[k] > 0 for k in tot if k != "skipped_by_n_un"), tot
    assert (tot["skipped_by_n_un"] > 0) == two


def test_node_size_case_has_exactly_its_size():
    for k1, k2, e2 in [(1, 1, 0), (40, 17, 0), (65, 600, 0), (40, 64, 9)]:
        S = bc.node_size_case(k1, k2, extra2=e2)
        st = br.search_by_bow_keyframes(S["kf1"], S["neighbours"][0])["stats"]
        assert st["eligible1"] == [k1] and st["eligible2"] == [k2] and st["node_sizes"] == [(k1 + 3, k2 + e2)]


def test_symbol_is_declared_and_exported():
    from fasttrack_amd import _capi
    assert "ft_search_by_bow_keyframes" in _capi.declared_symbols()
    assert hasattr(_capi.lib(), "ft_search_by_bow_keyframes")

"""The inputs of the ft_search_by_bow_candidates tests (tests/bow_reloc_cases.py) under the oracle's SearchByBoW(KeyFrame, Frame):
the committed scenarios exercise what they are meant to, the single-node cases have exactly their sizes, the hand-built expected
arrays are the oracle's, and the entry point is declared and exported.  No GPU."""
import numpy as np
import pytest

from tests import bow_reloc_cases as rc


def test_symbol_is_declared_and_exported():
    from fasttrack_amd import _capi
    assert "ft_search_by_bow_candidates" in _capi.declared_symbols()
    assert hasattr(_capi.lib(), "ft_search_by_bow_candidates")
    assert hasattr(_capi, "BowCandidate")


@pytest.mark.parametrize("i", range(len(rc.MAIN)))
def test_main_scenarios_are_not_vacuous(i):
    S = rc.main_scenario(i)
    two = rc.MAIN[i][1].get("two_cam", False)
    assert (S["nleft"] != -1) == two
    with_hist, loose, no_hist_loose = rc.oracle_main(i, (0.75, True)), rc.oracle_main(i, (0.9, True)), rc.oracle(S, 0.9, False)
    strict = rc.oracle_main(i, (0.6, False))
    removed = right = fewer = 0
    for k in range(len(S["candidates"])):
        for r in (with_hist[k], loose[k], strict[k]):
            assert r["n"] >= 15, (k, r["n"])  # the reference's own discard threshold (src/Tracking.cc:3847)
            assert r["n"] == int((r["matches"] >= 0).sum())
        removed += no_hist_loose[k]["n"] - loose[k]["n"]
        fewer += strict[k]["n"] < no_hist_loose[k]["n"]
        if two:
            right += int((with_hist[k]["matches"][S["nleft"]:] >= 0).sum())
    assert removed > 0 and fewer > 0
    assert (right > 0) == two


def test_the_long_node_takes_the_memory_path():
    S = rc.main_scenario(3)
    sizes = np.diff(S["frame"]["fv_offsets"])
    assert len(sizes) == 1 and sizes[0] > 256, sizes
    assert np.diff(rc.main_scenario(2)["frame"]["fv_offsets"]).max() <= 256


def test_degenerate_candidates_give_nothing():
    S = rc.scenario(51, n_k=(400, 500), empty_candidate=True, pointless_candidate=True, foreign_candidate=True)
    c = S["candidates"]
    assert len(c) == 5 and len(c[1]["descriptors"]) == 0 and not c[3]["has_point"].any()
    want = rc.oracle(S)
    assert [w["n"] >= 15 for w in want] == [True, False, True, False, False]
    for k in (1, 3, 4):
        assert want[k]["n"] == 0 and (want[k]["matches"] == -1).all()


def test_node_size_cases_have_exactly_their_sizes():
    for k_kf, k_f, two in [(40, 1, False), (40, 1, True), (40, 17, False), (40, 257, True), (130, 300, False), (1, 50, False)]:
        S = rc.node_size_case(k_kf, k_f, two)
        f, c = S["frame"], S["candidates"][0]
        assert f["fv_offsets"].tolist() == [0, k_f] and sorted(f["fv_features"].tolist()) == list(range(k_f))
        assert c["fv_offsets"].tolist() == [0, k_kf] and sorted(c["fv_features"].tolist()) == list(range(k_kf)) and c["has_point"].all()
        assert S["nleft"] == (int(0.55 * k_f) if two else -1)
        n = rc.oracle(S, 0.75, True)[0]["n"]
        if k_f == 1:
            assert n == (0 if two else 1)  # the only feature is a right-camera one: the left best stays 256
        elif k_kf >= 40 and k_f >= 15:
            assert n >= 6, (k_kf, k_f, two, n)


@pytest.mark.parametrize("case", rc.hand_built() + rc.rotation_cases(), ids=lambda c: c["name"])
def test_hand_built_cases(case):
    r = rc.oracle(case, case["nn_ratio"], case["check_orientation"])
    assert len(r) == len(case["candidates"]) >= 1
    for k in range(len(r)):
        assert np.array_equal(r[k]["matches"], case["matches"][k]) and r[k]["n"] == case["n"][k], (k, r[k]["matches"], r[k]["n"])

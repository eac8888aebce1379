"""ft_search_by_bow_keyframes on the device against the sequential restatement of ORBmatcher::SearchByBoW(KeyFrame, KeyFrame)
(tests/bow_kf_ref.py): matches12 and the counts equal, no tolerance and no excluded case.  Needs an MI355X."""
import functools

import numpy as np
import pytest

from fasttrack_amd import orb
from tests import bow_kf_cases as bc
from tests import bow_kf_ref as br

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def run(ctx, kf1, neighbours, nn_ratio=0.9, ori=True):
    return orb.search_by_bow_keyframes(ctx, bc.to_device(orb, kf1), [bc.to_device(orb, k) for k in neighbours], nn_ratio, ori)


def check(tag, got, want):
    assert got["matches12"].shape[0] == len(got["n"]) == len(want), tag
    for k, w in enumerate(want):
        assert np.array_equal(got["matches12"][k], w["matches12"]), (tag, k, np.nonzero(got["matches12"][k] != w["matches12"])[0][:10])
        assert int(got["n"][k]) == w["n"], (tag, k, int(got["n"][k]), w["n"])


@functools.lru_cache(maxsize=None)
def expected_main(i, cfg):
    S = bc.main_scenario(i)
    return [br.search_by_bow_keyframes(S["kf1"], nb, *cfg) for nb in S["neighbours"]]


@pytest.mark.parametrize("i", range(len(bc.MAIN)))
def test_scenarios_match_the_restatement(ctx, i):
    """three neighbours per call; ~100, ~10 and one node (700 x 700, the lists too long for the registers); one and two cameras"""
    S = bc.main_scenario(i)
    for cfg in bc.CONFIGS:
        want = expected_main(i, cfg)
        check((i, cfg), run(ctx, S["kf1"], S["neighbours"], *cfg), want)
        assert all(w["n"] >= 20 for w in want)
    if bc.MAIN[i][1]["levelsup"] == 4:
        assert expected_main(i, bc.CONFIGS[0])[0]["stats"]["node_sizes"][0][1] > 256


def _node_case(ctx, k1, k2, extra2=0):
    S = bc.node_size_case(k1, k2, extra2=extra2)
    for cfg in ((0.9, True), (0.7, False)):
        want = [br.search_by_bow_keyframes(S["kf1"], S["neighbours"][0], *cfg)]
        st = want[0]["stats"]
        assert st["eligible1"] == [k1] and st["eligible2"] == [k2] and st["node_sizes"] == [(k1 + 3, k2 + extra2)]
        check((k1, k2, extra2, cfg), run(ctx, S["kf1"], S["neighbours"], *cfg), want)


@pytest.mark.parametrize("k2", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600])
def test_candidate_counts(ctx, k2):
    """one node with exactly k2 eligible candidates: a single lane, the boundaries of a row of 16, of a wave, of the registers
    (256), the memory path"""
    _node_case(ctx, 40, k2)


@pytest.mark.parametrize("k2,extra2", [(16, 5), (60, 7), (250, 9), (256, 1), (300, 40)])
def test_candidate_counts_with_pointless_candidates(ctx, k2, extra2):
    """candidates without a map point inside the list: the list is longer than its eligible part"""
    _node_case(ctx, 40, k2, extra2)


@pytest.mark.parametrize("k1", [1, 63, 64, 65, 130])
def test_keyframe1_feature_counts(ctx, k1):
    """exactly k1 eligible keyframe-1 features in the node (they are loaded 64 at a time), against a short and a long list"""
    _node_case(ctx, k1, 50)
    _node_case(ctx, k1, 300)


def test_neighbour_counts_and_batching(ctx):
    """1, 3 and 5 neighbours per call, among the five an empty keyframe, one without map points and one without a shared node;
    the batched call equals the single calls"""
    S = bc.scenario(51, n2=(400, 500), empty_neighbour=True, pointless_neighbour=True, foreign_neighbour=True)
    nbs = S["neighbours"]
    assert len(nbs) == 5 and len(nbs[1]["descriptors"]) == 0 and not nbs[3]["has_point"].any()
    want = [br.search_by_bow_keyframes(S["kf1"], nb) for nb in nbs]
    assert [w["n"] > 20 for w in want] == [True, False, True, False, False]
    assert want[1]["n"] == want[3]["n"] == want[4]["n"] == 0 and want[4]["stats"]["shared_nodes"] == 0 and want[3]["stats"]["shared_nodes"] > 50
    g5 = run(ctx, S["kf1"], nbs)
    check(5, g5, want)
    for k in (1, 3, 4):
        assert (g5["matches12"][k] == -1).all()
    check(3, run(ctx, S["kf1"], nbs[:3]), want[:3])
    for k in range(5):
        g1 = run(ctx, S["kf1"], nbs[k:k + 1])
        check((1, k), g1, want[k:k + 1])
        assert np.array_equal(g1["matches12"][0], g5["matches12"][k])


@pytest.mark.parametrize("case", bc.hand_built() + bc.rotation_cases(), ids=lambda c: c["name"])
def test_hand_built_cases(ctx, case):
    g = run(ctx, case["kf1"], case["neighbours"], case["nn_ratio"], case["check_orientation"])
    assert np.array_equal(g["matches12"], case["matches12"]), g["matches12"]
    assert np.array_equal(g["n"], case["n"]), g["n"]


def test_launch_count_is_fixed(ctx):
    """two kernels per call, for one neighbour and for five"""
    S = bc.scenario(51, n2=(400, 500), empty_neighbour=True, pointless_neighbour=True, foreign_neighbour=True)
    try:
        ctx.set_kernel_timing(True)
        ctx.reset_stats()
        run(ctx, S["kf1"], S["neighbours"][:1])
        assert ctx.get_stat("search_by_bow_keyframes.launches") == (2.0, 1)
        run(ctx, S["kf1"], S["neighbours"])
        assert ctx.get_stat("search_by_bow_keyframes.launches") == (4.0, 2)
        for name in ("kernel.bow_kf_match", "kernel.bow_kf_finish"):
            assert ctx.get_stat(name)[1] == 2, name
    finally:
        ctx.set_kernel_timing(False)


def _empty(two_cam=False):
    return bc.keyframe(dict(fv_nodes=[], fv_offsets=[0], fv_features=[]), np.zeros((0, 32), np.uint8), [], [], 0 if two_cam else -1, 0)


def test_empty_inputs_return_without_a_launch(ctx):
    S = bc.main_scenario(0)
    ctx.reset_stats()
    g = run(ctx, _empty(), S["neighbours"])
    assert g["n"].tolist() == [0, 0, 0] and g["matches12"].shape == (3, 0)
    g = run(ctx, S["kf1"], [])
    assert len(g["n"]) == 0 and g["matches12"].shape == (0, len(S["kf1"]["descriptors"]))
    assert ctx.get_stat("search_by_bow_keyframes.launches") == (0.0, 0)


def test_bad_arguments_raise(ctx):
    S = bc.main_scenario(0)
    kf1, kf2 = S["kf1"], S["neighbours"][0]
    n2 = len(kf2["descriptors"])

    def bad(which=2, ori=True, **kw):
        a, b = (dict(kf1, **kw), kf2) if which == 1 else (kf1, dict(kf2, **kw))
        with pytest.raises(orb.FastTrackError) as e:
            run(ctx, a, [kf2, b], 0.9, ori)
        assert e.value.status == -1, kw

    nd = kf2["fv_nodes"].copy()
    nd[[2, 3]] = nd[[3, 2]]
    bad(fv_nodes=nd)                                             # fv_nodes not strictly ascending
    nd = kf1["fv_nodes"].copy()
    nd[1] = nd[0]
    bad(fv_nodes=nd, which=1)
    f = kf2["fv_features"].copy()
    f[3] = n2
    bad(fv_features=f)                                           # a feature index >= n
    f = kf2["fv_features"].copy()
    f[3] = f[4]
    bad(fv_features=f)                                           # a feature listed twice
    f = kf1["fv_features"].copy()
    f[0] = f[-1]
    bad(fv_features=f, which=1)
    bad(n_left=-2)                                               # n_left outside [-1, n]
    bad(n_left=n2 + 1)
    bad(n_left=n2 // 2, n_un=n2 + 1)                             # n_un outside [0, n] when n_left != -1
    bad(n_left=n2 // 2, n_un=-1)
    bad(n_left=10, n_un=-1, which=1)
    # check_orientation without angles, null arrays
    K1, K2 = bc.to_device(orb, kf1), bc.to_device(orb, kf2)

    def bad_raw(k1, k2s, ori):
        with pytest.raises(orb.FastTrackError) as e:
            orb.search_by_bow_keyframes(ctx, k1, k2s, 0.9, ori)
        assert e.value.status == -1

    no_angles = orb.BowKeyFrame(orb.BowSide(kf2["fv_nodes"], kf2["fv_offsets"], kf2["fv_features"], kf2["descriptors"], None), kf2["has_point"])
    bad_raw(K1, [K2, no_angles], True)
    bad_raw(no_angles, [K2], True)
    for field, side in (("has_point", False), ("descriptors", True), ("fv_features", True), ("fv_nodes", True), ("fv_offsets", True)):
        broken = bc.to_device(orb, kf2)
        setattr(broken.c.side if side else broken.c, field, None)
        bad_raw(K1, [K2, broken], False)
    # n_un is not read when n_left == -1, and angles are not needed without check_orientation
    want = [br.search_by_bow_keyframes(kf1, kf2, 0.9, False)]
    check("n_un ignored", run(ctx, kf1, [dict(kf2, n_un=-5)], 0.9, False), want)
    check("no angles", orb.search_by_bow_keyframes(ctx, K1, [no_angles], 0.9, False), want)
    check("after the errors", run(ctx, kf1, S["neighbours"]), expected_main(0, (0.9, True)))

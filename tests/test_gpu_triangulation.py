"""ft_search_for_triangulation on the device against the sequential restatement of ORBmatcher::SearchForTriangulation
(tests/triangulation_ref.py): matches12, n_matches and best_dist bit for bit, no tolerance and no excluded case."""
import functools

import numpy as np
import pytest

from fasttrack_amd import orb
from tests import triangulation_cases as tc
from tests import triangulation_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def run(ctx, S, flags=(False, False, True), neighbours=None):
    ks = S["neighbours"] if neighbours is None else [S["neighbours"][i] for i in neighbours]
    ps = S["pairs"] if neighbours is None else [S["pairs"][i] for i in neighbours]
    return orb.search_for_triangulation(ctx, tc.to_device(orb, S["kf1"]), [tc.to_device(orb, k) for k in ks],
                                        [tc.to_device_pair(orb, p) for p in ps], *flags)


@functools.lru_cache(maxsize=None)
def expected(key, flags):
    S = key() if callable(key) else tc.scenario(*key[0], **dict(key[1]))
    return [tr.search_for_triangulation(S["kf1"], k, p, *flags) for k, p in zip(S["neighbours"], S["pairs"])]


def check(tag, got, want):
    assert len(got["n"]) == len(want), tag
    for k, w in enumerate(want):
        assert np.array_equal(got["matches12"][k], w["matches12"]), (tag, k, np.nonzero(got["matches12"][k] != w["matches12"])[0][:10])
        assert int(got["n"][k]) == w["n"], (tag, k, int(got["n"][k]), w["n"])
        assert np.array_equal(got["best_dist"][k], w["best_dist"]), (tag, k)
        assert [tuple(r) for r in got["pairs"][k].tolist()] == w["pairs"], (tag, k)


FLAGS = {"pinhole": [(False, False, True), (False, True, True), (True, False, True), (False, False, False), (True, True, False)],
         "kb8": [(False, False, True), (False, True, False)], "kb8x2": [(False, False, True), (False, True, True), (True, False, True)]}


@pytest.mark.parametrize("form,seed,forward", tc.MAIN)
def test_scenarios_match_the_restatement(ctx, form, seed, forward):
    """three neighbours per call, every camera form, bOnlyStereo / bCoarse / mbCheckOrientation on and off"""
    key = ((form, seed), (("forward", forward),))
    S = tc.scenario(form, seed, forward=forward)
    for flags in FLAGS[form]:
        want = expected(key, flags)
        check((form, flags), run(ctx, S, flags), want)
        if flags == (False, False, True):
            assert all(w["n"] >= 100 for w in want)


@pytest.mark.parametrize("form", tc.FORMS)
@pytest.mark.parametrize("size", [1, 15, 16, 17, 63, 64, 65, 130])
def test_node_sizes(ctx, form, size):
    """one node with `size` candidates: a single lane, a full round of 16, rounds with a tail, several rounds"""
    S = tc.node_size_case(form, size, 21)
    want = [tr.search_for_triangulation(S["kf1"], S["neighbours"][0], S["pairs"][0])]
    assert want[0]["stats"]["node_sizes"] == {size}
    check((form, size), run(ctx, S), want)


@pytest.mark.parametrize("form", tc.FORMS)
def test_neighbour_counts_and_batching(ctx, form):
    """1, 3 and 5 neighbours per call, among them an empty keyframe and one without a shared node; the batched call equals the
    single calls; the first and the last feature of keyframe 1 are matched against some neighbour"""
    kw = dict(neighbours=3, empty_neighbour=True, foreign_neighbour=True)
    S = tc.scenario(form, 31, **kw)
    assert len(S["neighbours"]) == 5 and len(S["neighbours"][1]["keys"]) == 0
    want = expected(((form, 31), tuple(sorted(kw.items()))), (False, False, True))
    assert want[1]["n"] == 0 and want[4]["n"] == 0 and want[4]["stats"]["shared_nodes"] == 0 and want[0]["n"] >= 100
    g5 = run(ctx, S)
    check((form, 5), g5, want)
    assert (g5["matches12"][1] == -1).all() and (g5["best_dist"][4] == 50).all()
    check((form, 3), run(ctx, S, neighbours=[0, 1, 2]), want[:3])
    for k in range(5):
        g1 = run(ctx, S, neighbours=[k])
        check((form, 1, k), g1, want[k:k + 1])
        assert np.array_equal(g1["matches12"][0], g5["matches12"][k]) and np.array_equal(g1["best_dist"][0], g5["best_dist"][k])


def test_first_and_last_feature_are_matched(ctx):
    """every feature index of keyframe 1 is somebody's row: the first and the last one carry a match"""
    for c in tc.hand_built():
        if c["name"] == "no_orientation_check":
            S = dict(kf1=c["kf1"], neighbours=[c["kf2"]], pairs=[c["pair"]])
            g = run(ctx, S, c["flags"])
            assert g["matches12"][0][0] == 0 and g["matches12"][0][-1] == len(c["kf1"]["keys"]) - 1


@pytest.mark.parametrize("case", tc.hand_built(), ids=lambda c: c["name"])
def test_hand_built_cases(ctx, case):
    S = dict(kf1=case["kf1"], neighbours=[case["kf2"]], pairs=[case["pair"]])
    g = run(ctx, S, case["flags"])
    assert np.array_equal(g["matches12"][0], case["matches12"]), g["matches12"][0]
    assert int(g["n"][0]) == case["n"] and np.array_equal(g["best_dist"][0], case["best_dist"]), (g["n"], g["best_dist"][0])


@pytest.mark.parametrize("case", tc.rotation_cases(), ids=lambda c: c["name"])
def test_rotation_cases(ctx, case):
    """the directed histograms the matchers share, one per call and all as the neighbours of one call"""
    g = run(ctx, case, case["flags"])
    assert np.array_equal(g["matches12"], case["matches12"]), g["matches12"]
    assert np.array_equal(g["n"], case["n"]) and np.array_equal(g["best_dist"], case["best_dist"]), (g["n"], g["best_dist"])


def test_the_four_pairings(ctx):
    kf1, kf2, P = tc.four_pairings()
    S = dict(kf1=kf1, neighbours=[kf2], pairs=[P])
    for flags in ((False, False, False), (False, True, False)):
        check(flags, run(ctx, S, flags), [tr.search_for_triangulation(kf1, kf2, P, *flags)])


def test_launch_count_is_fixed(ctx):
    """two kernels per call, for one neighbour and for five"""
    S = tc.scenario("pinhole", 31, neighbours=3, empty_neighbour=True, foreign_neighbour=True)
    try:
        ctx.set_kernel_timing(True)
        ctx.reset_stats()
        run(ctx, S, neighbours=[0])
        assert ctx.get_stat("search_for_triangulation.launches") == (2.0, 1)
        run(ctx, S)
        assert ctx.get_stat("search_for_triangulation.launches") == (4.0, 2)
        for name in ("kernel.triang_match", "kernel.triang_finish"):
            assert ctx.get_stat(name)[1] == 2, name
    finally:
        ctx.set_kernel_timing(False)


def test_empty_inputs_return_without_a_launch(ctx):
    S = tc.scenario("pinhole", 11)
    empty = tc.keyframe(tc._keys([], [], []), np.zeros((0, 32), np.uint8), dict(fv_nodes=[], fv_offsets=[0], fv_features=[]), [], 0, tc.PINHOLE_CAM)
    ctx.reset_stats()
    g = run(ctx, dict(kf1=empty, neighbours=S["neighbours"], pairs=S["pairs"]))
    assert g["n"].tolist() == [0, 0, 0] and g["matches12"].shape == (3, 0)
    g = run(ctx, dict(kf1=S["kf1"], neighbours=[], pairs=[]))
    assert len(g["n"]) == 0 and g["pairs"] == []
    assert ctx.get_stat("search_for_triangulation.launches") == (0.0, 0)


def test_bad_arguments_raise(ctx):
    S = tc.scenario("pinhole", 11)
    kf1, kf2, P = S["kf1"], S["neighbours"][0], S["pairs"][0]

    def bad(**kw):
        which = kw.pop("which", 2)
        a, b = (dict(kf1, **kw), kf2) if which == 1 else (kf1, dict(kf2, **kw))
        with pytest.raises(orb.FastTrackError) as e:
            run(ctx, dict(kf1=a, neighbours=[b], pairs=[P]))
        assert e.value.status == -1, kw
    bad(two_cameras=True)                                        # a pinhole keyframe with two cameras
    bad(cam_model=1)                                             # the keyframes of a call differ in the camera model
    bad(cam_model=1, two_cameras=True)                           # ... and in two_cameras
    f = kf2["fv_features"].copy()
    f[3] = len(kf2["keys"])
    bad(fv_features=f)                                           # a feature index >= n
    f = kf2["fv_features"].copy()
    f[3] = f[4]
    bad(fv_features=f)                                           # a feature listed twice
    k = kf2["keys"].copy()
    k["octave"][5] = tc.NLEVELS
    bad(keys=k)                                                  # an octave outside [0, nlevels)
    k = kf1["keys"].copy()
    k["octave"][0] = -1
    bad(keys=k, which=1)
    nd = kf2["fv_nodes"].copy()
    nd[[2, 3]] = nd[[3, 2]]
    bad(fv_nodes=nd)                                             # unsorted fv_nodes
    nd = kf1["fv_nodes"].copy()
    nd[1] = nd[0]
    bad(fv_nodes=nd, which=1)
    check("after the errors", run(ctx, S), expected((("pinhole", 11), ()), (False, False, True)))

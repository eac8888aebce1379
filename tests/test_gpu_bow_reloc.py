"""ft_search_by_bow_candidates on the device against the oracle's SearchByBoW(KeyFrame, Frame), one oracle call per candidate:
rows and counts equal, no tolerance and no excluded case.  Needs an MI355X."""
import numpy as np
import pytest

from fasttrack_amd import orb
from tests import bow_reloc_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def run(ctx, S, nn_ratio=0.75, ori=True, candidates=None, **kw):
    frame, cands = rc.to_device(orb, S, candidates)
    return orb.search_by_bow_candidates(ctx, frame, cands, S["nleft"], nn_ratio, ori, **kw)


def check(tag, got, want):
    assert got["matches"].shape[0] == len(got["n"]) == len(want), tag
    for k, w in enumerate(want):
        assert np.array_equal(got["matches"][k], w["matches"]), (tag, k, np.nonzero(got["matches"][k] != w["matches"])[0][:10])
        assert int(got["n"][k]) == w["n"], (tag, k, int(got["n"][k]), w["n"])


def single(ctx, S, c, nn_ratio=0.75, ori=True):
    """ft_search_by_bow for one candidate: the row the batched call must reproduce"""
    mk = lambda s: orb.BowSide(s["fv_nodes"], s["fv_offsets"], s["fv_features"], s["descriptors"], s["angles"])
    return orb.search_by_bow(ctx, mk(c), c["has_point"], mk(S["frame"]), S["nleft"], nn_ratio, ori)


@pytest.mark.parametrize("i", range(len(rc.MAIN)))
def test_scenarios_match_the_oracle(ctx, i):
    """four candidates per call (two on the 690-feature node); ~100, 10 and one node; one and two cameras"""
    S = rc.main_scenario(i)
    for cfg in rc.CONFIGS:
        want = rc.oracle_main(i, cfg)
        check((i, cfg), run(ctx, S, *cfg), want)
        assert all(w["n"] >= 15 for w in want)


def _node_case(ctx, k_kf, k_f, two_cam):
    S = rc.node_size_case(k_kf, k_f, two_cam)
    assert np.diff(S["frame"]["fv_offsets"]).tolist() == [k_f] and np.diff(S["candidates"][0]["fv_offsets"]).tolist() == [k_kf]
    for cfg in ((0.75, True), (0.6, False)):
        check((k_kf, k_f, two_cam, cfg), run(ctx, S, *cfg), rc.oracle(S, *cfg))


@pytest.mark.parametrize("two_cam", [False, True])
@pytest.mark.parametrize("k_f", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600])
def test_frame_node_sizes(ctx, k_f, two_cam):
    """one node with exactly k_f frame features: a single lane, the boundaries of a row of 16, of a wave, of the four register
    rounds (256), the memory path"""
    _node_case(ctx, 40, k_f, two_cam)


@pytest.mark.parametrize("k_kf", [1, 63, 64, 65, 130])
def test_candidate_list_sizes(ctx, k_kf):
    """exactly k_kf candidate features in the node (they are loaded 64 at a time), against a short and a long frame node"""
    _node_case(ctx, k_kf, 50, False)
    _node_case(ctx, k_kf, 300, False)


def test_candidate_counts_and_batching(ctx):
    """1, 3 and 5 candidates per call, among the five an empty keyframe, one without map points and one without a shared node;
    every row of the batched call equals the single-candidate call and ft_search_by_bow"""
    S = rc.scenario(51, n_k=(400, 500), empty_candidate=True, pointless_candidate=True, foreign_candidate=True)
    cs = S["candidates"]
    assert len(cs) == 5 and len(cs[1]["descriptors"]) == 0 and not cs[3]["has_point"].any()
    want = rc.oracle(S)
    assert [w["n"] >= 15 for w in want] == [True, False, True, False, False]
    g5 = run(ctx, S)
    check(5, g5, want)
    for k in (1, 3, 4):
        assert (g5["matches"][k] == -1).all() and g5["n"][k] == 0
    check(3, run(ctx, S, candidates=cs[:3]), want[:3])
    for k in range(5):
        g1 = run(ctx, S, candidates=cs[k:k + 1])
        check((1, k), g1, want[k:k + 1])
        assert np.array_equal(g1["matches"][0], g5["matches"][k])
        s = single(ctx, S, cs[k])
        assert np.array_equal(s["matches"], g5["matches"][k]) and s["n"] == g5["n"][k], k


@pytest.mark.parametrize("i", [1, 3])
def test_no_claim_crosses_candidates(ctx, i):
    """the same candidate three times in one call gives three identical rows: on register-resident nodes (two cameras) and on the
    690-feature node, whose claims live in the rows themselves"""
    S = rc.main_scenario(i)
    c = S["candidates"][0]
    want = rc.oracle_main(i, (0.75, True))[0]
    g = run(ctx, S, candidates=[c, c, c])
    check(("thrice", i), g, [want] * 3)
    # ... and next to a different one on either side
    other = S["candidates"][1]
    check(("mixed", i), run(ctx, S, candidates=[other, c, other]), [rc.oracle_main(i, (0.75, True))[k] for k in (1, 0, 1)])


def test_seventy_candidates_in_one_call(ctx):
    S = rc.many_small()
    assert len(S["candidates"]) == 70
    want = rc.oracle(S)
    assert sum(w["n"] for w in want) > 70 * 15
    check(70, run(ctx, S), want)


@pytest.mark.parametrize("case", rc.hand_built() + rc.rotation_cases(), ids=lambda c: c["name"])
def test_hand_built_cases(ctx, case):
    g = run(ctx, case, case["nn_ratio"], case["check_orientation"])
    assert np.array_equal(g["matches"], case["matches"]), g["matches"]
    assert np.array_equal(g["n"], case["n"]), g["n"]


@pytest.mark.parametrize("case", rc.rotation_cases(), ids=lambda c: c["name"])
def test_rotation_cases_through_search_by_bow(ctx, case):
    """the same frame / candidate pairs through ft_search_by_bow, whose filter is the host's (rot_hist.h): the hand-listed rows pin
    the host twin and the device twin against each other"""
    for k, c in enumerate(case["candidates"]):
        s = single(ctx, case, c, case["nn_ratio"], case["check_orientation"])
        assert np.array_equal(s["matches"], case["matches"][k]) and s["n"] == case["n"][k], (k, s["matches"], s["n"])


@pytest.mark.parametrize("i", [1, 3])
def test_resident_frame_descriptors(ctx, i):
    """the frame's descriptors in ft_device_malloc memory: the same result, and the copy up is smaller by their bytes"""
    S = rc.main_scenario(i)
    n_f = len(S["frame"]["descriptors"])
    buf = ctx.to_device(S["frame"]["descriptors"])
    try:
        ctx.reset_stats()
        host = run(ctx, S)
        up_host = ctx.get_stat("search_by_bow_candidates.up_bytes")
        ctx.reset_stats()
        dev = run(ctx, S, frame_device_ptr=buf)
        up_dev = ctx.get_stat("search_by_bow_candidates.up_bytes")
    finally:
        buf.free()
    check(("resident", i), dev, rc.oracle_main(i, (0.75, True)))
    assert np.array_equal(dev["matches"], host["matches"]) and np.array_equal(dev["n"], host["n"])
    assert up_host[1] == up_dev[1] == 1
    assert up_host[0] - up_dev[0] == (32 * n_f + 63) // 64 * 64, (up_host, up_dev)


def test_launch_count_is_fixed(ctx):
    """two kernels per call, for one candidate and for five"""
    S = rc.scenario(51, n_k=(400, 500), empty_candidate=True, pointless_candidate=True, foreign_candidate=True)
    try:
        ctx.set_kernel_timing(True)
        ctx.reset_stats()
        run(ctx, S, candidates=S["candidates"][:1])
        assert ctx.get_stat("search_by_bow_candidates.launches") == (2.0, 1)
        run(ctx, S)
        assert ctx.get_stat("search_by_bow_candidates.launches") == (4.0, 2)
        for name in ("kernel.bow_cand_match", "kernel.bow_cand_finish"):
            assert ctx.get_stat(name)[1] == 2, name
        assert ctx.get_stat("search_by_bow_candidates.total")[1] == 2
    finally:
        ctx.set_kernel_timing(False)


def test_empty_inputs_return_without_a_launch(ctx):
    S = rc.main_scenario(0)
    ctx.reset_stats()
    empty = dict(S, frame=rc.side(rc.EMPTY_FV, np.zeros((0, 32), np.uint8), []))
    g = run(ctx, empty)
    assert g["n"].tolist() == [0, 0, 0, 0] and g["matches"].shape == (4, 0)
    g = run(ctx, S, candidates=[])
    assert len(g["n"]) == 0 and g["matches"].shape == (0, len(S["frame"]["descriptors"]))
    assert ctx.get_stat("search_by_bow_candidates.launches") == (0.0, 0)


def test_bad_arguments_raise_and_write_nothing(ctx):
    S = rc.main_scenario(0)
    f, c0, c1 = S["frame"], S["candidates"][0], S["candidates"][1]
    n_f, n1 = len(f["descriptors"]), len(c1["descriptors"])
    from fasttrack_amd import _capi
    import ctypes as C

    def raw(frame, cands, nleft=-1, ori=True, n_keyframes=None, null_matches=False, null_counts=False):
        """the C call with sentinel-filled outputs: -1 (FT_ERR_INVALID) and nothing written"""
        K = (_capi.BowCandidate * max(len(cands), 1))(*[k.c for k in cands])
        m = np.full(max(len(cands) * frame.c.n, 1), 12345, np.int32)
        cnt = np.full(max(len(cands), 1), 777, np.int32)
        st = _capi.lib().ft_search_by_bow_candidates(ctx._h, C.byref(frame.c), nleft, 0, len(cands) if n_keyframes is None else n_keyframes, K,
                                                     0.75, int(ori), None if null_matches else orb.ptr(m), None if null_counts else orb.ptr(cnt))
        assert st == -1, st
        assert (m == 12345).all() and (cnt == 777).all()

    def bad(which, ori=True, nleft=-1, **kw):
        Sb = dict(S, frame=dict(f, **kw)) if which == "frame" else S
        cands = [c0, dict(c1, **kw)] if which == "candidate" else [c0, c1]
        F, K = rc.to_device(orb, Sb, cands)
        raw(F, K, nleft, ori)
        with pytest.raises(orb.FastTrackError) as e:
            orb.search_by_bow_candidates(ctx, F, K, nleft, 0.75, ori)
        assert e.value.status == -1, kw

    for which, s in (("frame", f), ("candidate", c1)):
        nd = s["fv_nodes"].copy()
        nd[[2, 3]] = nd[[3, 2]]
        bad(which, fv_nodes=nd)                                    # fv_nodes not strictly ascending
        ft = s["fv_features"].copy()
        ft[3] = len(s["descriptors"])
        bad(which, fv_features=ft)                                 # a feature index >= n
        off = s["fv_offsets"].copy()
        off[0] = 1
        bad(which, fv_offsets=off)                                 # fv_offsets[0] != 0
        off = s["fv_offsets"].copy()
        off[2] = off[3] + 1
        bad(which, fv_offsets=off)                                 # fv_offsets not ascending
    ft = f["fv_features"].copy()
    ft[3] = ft[4]
    bad("frame", fv_features=ft)                                   # a frame feature listed twice
    bad("none", nleft=-2)                                          # frame_nleft outside [-1, n]
    bad("none", nleft=n_f + 1)
    F, K = rc.to_device(orb, S, [c0, c1])
    mk = lambda s, ang: orb.BowSide(s["fv_nodes"], s["fv_offsets"], s["fv_features"], s["descriptors"], ang)
    no_angles_c = orb.BowCandidate(mk(c1, None), c1["has_point"])
    raw(F, [K[0], no_angles_c])                                    # check_orientation without angles
    raw(mk(f, None), K)
    for field, in_side in (("has_point", False), ("descriptors", True), ("fv_features", True), ("fv_nodes", True), ("fv_offsets", True)):
        broken = rc.to_device(orb, S, [c1])[1][0]
        setattr(broken.c.side if in_side else broken.c, field, None)
        raw(F, [K[0], broken], ori=False)
    for field in ("descriptors", "fv_features", "fv_nodes", "fv_offsets"):
        Fb = rc.to_device(orb, S, [])[0]
        setattr(Fb.c, field, None)
        raw(Fb, K, ori=False)
    for field in ("n", "n_nodes"):                                 # counts out of range
        Fb = rc.to_device(orb, S, [])[0]
        setattr(Fb.c, field, -1)
        raw(Fb, K, ori=False)
        broken = rc.to_device(orb, S, [c1])[1][0]
        setattr(broken.c.side, field, -1)
        raw(F, [K[0], broken], ori=False)
    short = rc.to_device(orb, S, [c1])[1][0]
    short.c.side.n = int(c1["fv_offsets"][-1]) - 1                 # more FeatureVector entries than features
    raw(F, [K[0], short], ori=False)
    raw(F, K, n_keyframes=-1)                                      # n_keyframes outside [0, 65535]
    raw(F, K, n_keyframes=65536)
    raw(F, K, null_matches=True)                                   # null outputs with something to write
    raw(F, K, null_counts=True)
    # angles are not needed without check_orientation; and a valid call after the errors is still right
    want = rc.oracle(S, 0.75, False, [c1])
    check("no angles", orb.search_by_bow_candidates(ctx, mk(f, None), [no_angles_c], -1, 0.75, False), want)
    check("after the errors", run(ctx, S), rc.oracle_main(0, (0.75, True)))
    assert n1 > 0

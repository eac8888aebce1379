"""ft_search_keyframe_sim3 against the restatement of ORBmatcher::SearchByProjection(pKF, Scw, ...) (tests/sim3_search_ref.py, held
to its second formulation and to the hand-built expectations by test_sim3_search_cpu.py), bit for bit: vpMatched, the keypoint every
point wrote, the exit code of every point and the return value.  Needs an MI355X.

The inputs are those of tests/sim3_cases.py; what they exercise is asserted in test_sim3_search_cpu.py.  Every case holds a few
hundred keypoints and at most 3 500 points."""
import ctypes as C

import numpy as np
import pytest

from fasttrack_amd import _capi, orb
from oracle import binding as ob
from tests import sim3_cases as s3
from tests import sim3_search_ref as ref

pytestmark = pytest.mark.gpu
FIELDS = ("matched", "point_keypoint", "stage")


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def same(tag, g, r):
    for f in FIELDS:
        bad = np.nonzero(g[f] != r[f])[0]
        assert len(bad) == 0, f"{tag}: {f} differs at {bad[:5].tolist()}: {g[f][bad[:5]].tolist()} != {r[f][bad[:5]].tolist()}"
    assert g["n_matches"] == r["n_matches"], f"{tag}: n_matches {g['n_matches']} != {r['n_matches']}"


@pytest.mark.parametrize("name,th,ratio,hand", s3.USED)
def test_random_case(ctx, name, th, ratio, hand):
    """both overloads at (8, 1.5), (5, 1.0), (3, 1.5); pinhole, KannalaBrandt8 with one and two cameras; shifted bounds (fractional
    mnMinX, keypoints outside the grid) and pyramids of 1 - 12 levels"""
    case = s3.random_case(name)
    r = s3.expected(case, th, ratio, hand)
    g = orb.search_keyframe_sim3(ctx, case["view"]()[1], [s3.job_of(case, th, ratio, hand)])[0]
    same(f"{name} th {th} ratio {ratio} hand {hand}", g, r)
    assert r["n_matches"] >= 50
    assert np.array_equal(g["matched"][case["nleft"]:], case["matched"][case["nleft"]:])


def three_jobs(case):
    """the :755 -> :777 chain - (8, 1.5) written out, then (5, 1.0) through mpCamera->project on what the first left - and a third job
    of another M, valid and threshold"""
    first = s3.expected(case, 8, 1.5, True)
    M3 = len(case["valid"]) // 3 + 5
    pts3 = {k: v[:M3] for k, v in case["points"].items()}
    valid3 = np.roll(case["valid"], 7)[:M3]
    jobs = [s3.job_of(case, 8, 1.5, True), s3.job_of(case, 5, 1.0, False, matched=first["matched"]),
            s3.job_of(case, 3, 1.5, False, points=pts3, valid=valid3)]
    refs = [first, s3.expected(case, 5, 1.0, False, matched=first["matched"], tag="chained"),
            s3.expected(case, 3, 1.5, False, tag="third", points=pts3, valid=valid3)]
    return jobs, refs


@pytest.mark.parametrize("name", [s3.RANDOM[0], "kb8two"])
def test_three_jobs_equal_three_calls(ctx, name):
    case = s3.random_case(name)
    jobs, refs = three_jobs(case)
    _, gF = case["view"]()
    ctx.reset_stats()
    g = orb.search_keyframe_sim3(ctx, gF, jobs)
    total3, calls3 = ctx.get_stat("sim3.launches")
    for k, r in enumerate(refs):
        same(f"job {k} of 3", g[k], r)
    # (the chained job finds little: the first one has taken most of what its points want)
    assert refs[0]["n_matches"] >= 50 and min(r["n_matches"] for r in refs) >= 1
    assert not np.array_equal(refs[1]["point_keypoint"], s3.expected(case, 5, 1.0, False)["point_keypoint"])
    ctx.reset_stats()
    for k, j in enumerate(jobs):
        s = orb.search_keyframe_sim3(ctx, gF, [j])[0]
        same(f"job {k} alone", s, g[k])
    total1, calls1 = ctx.get_stat("sim3.launches")
    # the number of launches per call does not depend on the number of jobs
    assert calls3 == 1 and calls1 == 3 and total3 == total1 / 3 == 3


@pytest.mark.parametrize("name", sorted(s3.hand_cases()))
def test_hand_case(ctx, name):
    case = s3.hand_cases()[name]
    _, gF = s3.hand_view(case["keys"], case["desc"], device=True, keys_right=case["keys_right"])
    for hand in (False, True):
        r = s3.run_hand_case(case, hand_pinhole=hand)
        g = orb.search_keyframe_sim3(ctx, gF, [s3.hand_job(case, hand)])[0]
        same(name, g, r)
        for f in FIELDS:
            assert g[f].tolist() == case["expect"][f], (name, hand, f)
        assert g["n_matches"] == case["expect"]["n_matches"]


def test_the_overloads_differ_on_a_window_edge(ctx):
    case, seen_by_hand = s3.overload_case()
    _, gF = s3.hand_view(case["keys"], case["desc"], device=True)
    g = orb.search_keyframe_sim3(ctx, gF, [s3.hand_job(case, False), s3.hand_job(case, True)])
    for hand in (False, True):
        same(f"hand {hand}", g[hand], s3.run_hand_case(case, hand_pinhole=hand))
    assert g[seen_by_hand]["matched"].tolist() == [0] and g[not seen_by_hand]["matched"].tolist() == [-1]
    assert g[not seen_by_hand]["stage"].tolist() == [ref.EMPTY]


@pytest.mark.parametrize("n", [4, 5, 16, 17, 65, 130])
def test_crowded_cell(ctx, n):
    """more candidates within the threshold than the top record holds: from the fifth point on the window is scanned again, in
    rounds of 64 entries with and without a tail"""
    case = s3.crowd_case(n)
    r = s3.run_hand_case(case)
    _, gF = s3.hand_view(case["keys"], case["desc"], device=True)
    g = orb.search_keyframe_sim3(ctx, gF, [s3.hand_job(case)])[0]
    same(f"crowd {n}", g, r)
    assert g["n_matches"] == n


@pytest.mark.parametrize("M", [1, 15, 16, 17, 1023, 1024, 1025])
def test_point_counts(ctx, M):
    """rows of a workgroup (16) and chunks of the compaction (1024) with and without a tail"""
    case = s3.random_case(s3.RANDOM[0])
    pts = {k: v[:M] for k, v in case["points"].items()}
    r = s3.expected(case, 8, 1.5, True, tag=("M", M), points=pts, valid=case["valid"][:M])
    g = orb.search_keyframe_sim3(ctx, case["view"]()[1], [s3.job_of(case, 8, 1.5, True, points=pts, valid=case["valid"][:M])])[0]
    same(f"M {M}", g, r)


def test_empty_inputs_launch_nothing(ctx):
    case = s3.random_case(s3.RANDOM[0])
    oF, gF = case["view"]()
    M = len(case["valid"])
    none = {k: v[:0] for k, v in case["points"].items()}
    kw = dict(keys=np.zeros(0, ob.KP_DTYPE), descriptors=np.zeros((0, 32), np.uint8), bounds=s3.fc.sc.frame_bounds(320, 240),
              cam=[oF.c.cam[i] for i in range(8)])
    eF = orb.FrameView(scale_factors=gF.sf, **kw)
    ctx.reset_stats()
    assert orb.search_keyframe_sim3(ctx, gF, []) == []
    g = orb.search_keyframe_sim3(ctx, gF, [s3.job_of(case, 8, 1.5, True, points=none, valid=None)] * 2)
    for k in range(2):
        assert g[k]["n_matches"] == 0 and np.array_equal(g[k]["matched"], case["matched"]) and g[k]["point_keypoint"].shape == (0,)
    g = orb.search_keyframe_sim3(ctx, eF, [dict(s3.job_of(case, 8, 1.5, True), matched=np.zeros(0, np.int32))])[0]
    assert g["n_matches"] == 0 and (g["point_keypoint"] == -1).all() and len(g["point_keypoint"]) == M and (g["stage"] == ref.EMPTY).all()
    assert ctx.get_stat("sim3.launches") == (0.0, 0)
    # an empty job beside a full one; nothing valid
    g = orb.search_keyframe_sim3(ctx, gF, [s3.job_of(case, 8, 1.5, True, points=none, valid=None), s3.job_of(case, 8, 1.5, True),
                                           s3.job_of(case, 8, 1.5, True, valid=np.zeros(M, np.uint8))])
    assert g[0]["n_matches"] == 0 and np.array_equal(g[0]["matched"], case["matched"])
    same("beside an empty job", g[1], s3.expected(case, 8, 1.5, True))
    assert g[2]["n_matches"] == 0 and np.array_equal(g[2]["matched"], case["matched"]) and (g[2]["stage"] == ref.SKIPPED).all()
    assert ctx.get_stat("sim3.launches") == (3.0, 1)


def test_outputs_may_be_null(ctx):
    case = s3.random_case("kb8mono")
    r = s3.expected(case, 5, 1.0, False)
    g = orb.search_keyframe_sim3(ctx, case["view"]()[1], [s3.job_of(case, 5, 1.0, False)], want_stage=False, want_point_keypoint=False)[0]
    assert g["stage"] is None and g["point_keypoint"] is None
    assert np.array_equal(g["matched"], r["matched"]) and g["n_matches"] == r["n_matches"]


def test_invalid_arguments(ctx):
    case = s3.random_case(s3.RANDOM[0])

    def bad(gF, job, status=_capi.FT_ERR_INVALID):
        with pytest.raises(orb.FastTrackError) as e:
            orb.search_keyframe_sim3(ctx, gF, [s3.job_of(case, 5, 1.0, False), job])   # (beside a good job: nothing of either is run)
        assert e.value.status == status

    _, gF = case["view"]()
    good = s3.job_of(case, 8, 1.5, True)
    bad(gF, dict(good, th=0))
    bad(gF, dict(good, ratio_hamming=5.12))            # 50 * 5.12f = 256: the reference would write vpMatched[-1]
    bad(gF, dict(good, ratio_hamming=-0.01))
    bad(gF, dict(good, ratio_hamming=float("nan")))
    bad(gF, dict(good, Tcw=orb.SE3([0, 0, 0, 2], [0, 0, 0])))
    _, wF = case["view"]()
    wF.c.cam_model = 7
    bad(wF, good)
    hand = s3.hand_cases()["match"]
    _, hF = s3.hand_view(s3.hand_keys([(300, 220)], octave=[8]), hand["desc"], device=True)
    with pytest.raises(orb.FastTrackError) as e:
        orb.search_keyframe_sim3(ctx, hF, [s3.hand_job(hand)])
    assert e.value.status == _capi.FT_ERR_INVALID
    # null arrays: the points' normals, matched, the jobs
    keep = {k: np.ascontiguousarray(v) for k, v in case["points"].items()}
    matched = case["matched"].copy()
    J = (_capi.Sim3Job * 1)()
    P = J[0].points
    P.M = len(case["valid"])
    P.world_pos, P.normal = _capi.ptr(keep["world_pos"]), None
    P.max_distance, P.min_distance, P.descriptors = _capi.ptr(keep["max_distance"]), _capi.ptr(keep["min_distance"]), _capi.ptr(keep["descriptors"])
    J[0].Tcw = orb.SE3(case["Tcw"].q, case["Tcw"].t).c
    J[0].Ow[:] = [float(v) for v in case["Ow"]]
    J[0].log_scale_factor, J[0].th, J[0].ratio_hamming, J[0].hand_pinhole = case["log_sf"], 8, 1.5, 1
    J[0].matched, J[0].n_matches = _capi.ptr(matched), 7
    L = _capi.lib()
    assert L.ft_search_keyframe_sim3(ctx._h, C.byref(gF.c), 1, J) == _capi.FT_ERR_INVALID
    P.normal, J[0].matched = _capi.ptr(keep["normal"]), None
    assert L.ft_search_keyframe_sim3(ctx._h, C.byref(gF.c), 1, J) == _capi.FT_ERR_INVALID
    J[0].matched = _capi.ptr(matched)
    assert L.ft_search_keyframe_sim3(ctx._h, C.byref(gF.c), 1, None) == _capi.FT_ERR_INVALID
    assert L.ft_search_keyframe_sim3(ctx._h, None, 1, J) == _capi.FT_ERR_INVALID
    assert J[0].n_matches == 7 and np.array_equal(matched, case["matched"])
    assert L.ft_search_keyframe_sim3(ctx._h, C.byref(gF.c), 1, J) == 0      # and the same call complete (valid NULL: every point)
    r = s3.expected(case, 8, 1.5, True, tag="all valid", valid=None)
    assert J[0].n_matches == r["n_matches"] and np.array_equal(matched, r["matched"])


def test_capacity_is_a_taken_bit_per_keypoint(ctx):
    """more left keypoints than the resolution has taken bits for: FT_ERR_CAPACITY before anything runs, nothing written"""
    n = 150 * 1024 * 8 + 1
    keys = np.zeros(n, ob.KP_DTYPE)
    keys["x"], keys["y"] = 100.0, 100.0
    hand = s3.hand_cases()["match"]
    kw = dict(keys=keys, descriptors=np.zeros((n, 32), np.uint8), bounds=(0, 0, s3.fc.W, s3.fc.H), cam=s3.fc.CAM)
    big = orb.FrameView(scale_factors=s3.fc.SF, **kw)
    matched = np.full(n, -1, np.int32)
    J = (_capi.Sim3Job * 1)()
    keep = {k: np.ascontiguousarray(v) for k, v in hand["points"].items()}
    P = J[0].points
    P.M = 1
    P.world_pos, P.normal, P.descriptors = _capi.ptr(keep["world_pos"]), _capi.ptr(keep["normal"]), _capi.ptr(keep["descriptors"])
    P.max_distance, P.min_distance = _capi.ptr(keep["max_distance"]), _capi.ptr(keep["min_distance"])
    J[0].Tcw = orb.SE3(s3.IDENTITY.q, s3.IDENTITY.t).c
    pk, st = np.full(1, 7, np.int32), np.full(1, 9, np.uint8)
    J[0].log_scale_factor, J[0].th, J[0].ratio_hamming = s3.LOG_SF, 3, 1.0
    J[0].matched, J[0].point_keypoint, J[0].stage, J[0].n_matches = _capi.ptr(matched), _capi.ptr(pk), _capi.ptr(st), 7
    ctx.reset_stats()
    assert _capi.lib().ft_search_keyframe_sim3(ctx._h, C.byref(big.c), 1, J) == _capi.FT_ERR_CAPACITY
    assert J[0].n_matches == 7 and pk[0] == 7 and st[0] == 9 and (matched == -1).all() and ctx.get_stat("sim3.launches") == (0.0, 0)

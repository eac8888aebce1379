"""ft_search_keyframe_projection / ft_tracked_frame_search_keyframe_projection against the restatement of
ORBmatcher::SearchByProjection(Frame, KeyFrame, sAlreadyFound, th, ORBdist) (tests/reloc_search_ref.py, pinned against the oracle by
test_reloc_search_cpu.py), bit for bit: assign, nmatches, holder_obs, bestDist, bestIdx2.  Needs an MI355X.

The inputs are those of tests/reloc_cases.py; what the restatement reports on them is listed in test_reloc_search_cpu.py and
asserted there and in test_inputs_exercise_the_sequential_part below.  Every case holds a few hundred keypoints."""
import numpy as np
import pytest

from fasttrack_amd import orb
from oracle import binding as ob
from tests import reloc_cases as rc
from tests import reloc_search_ref as ref
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

P320 = "pinhole:320x240:500:5"
GEOMETRY = [("loose", 1.2, 8), ("tight", 1.2, 8), ("edge", 1.2, 8), ("tight", 1.2, 1), ("tight", 2.0, 2), ("tight", 1.5, 5), ("tight", 1.1, 12)]


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tf(ctx):
    t = orb.TrackedFrame(ctx, 4096, 4096)
    yield t
    t.close()


def se3(T: "ob.SE3"):
    return orb.SE3(T.q, T.t)


def check_against_ref(tag, g, r, holder, with_best=True):
    assert g["n"] == r["n"], f"{tag}: n_matches {g['n']} != {r['n']}"
    assert np.array_equal(g["assign"], r["assign"]), f"{tag}: assign"
    assert np.array_equal(holder, r["holder_obs"]), f"{tag}: holder_obs"
    if with_best:
        assert np.array_equal(g["best_dist"], r["best_dist"]), f"{tag}: best_dist"
        assert np.array_equal(g["best_idx"], r["best_idx"]), f"{tag}: best_idx"


def run_both(ctx, tf, gF_of, kf, Tcw, log_sf, th, orb_dist, ori):
    """the non-resident entry and the resident entry on fresh device views -> (g, its holder_obs, t, its holder_obs)"""
    gF = gF_of()
    g = orb.KernelController.search_keyframe_projection(ctx, gF, kf, se3(Tcw), log_sf, th, orb_dist, ori)
    tf.upload(gF_of())
    t = tf.search_keyframe_projection(kf, se3(Tcw), log_sf, th, orb_dist, ori)
    return g, gF.holder_obs.copy(), t, tf.holder_obs()


def check_case(ctx, tf, tag, case, th, orb_dist, ori, uright=True, min_n=1):
    r = rc.expected(case, th, orb_dist, ori)
    g, gh, t, th_ = run_both(ctx, tf, lambda: case["view"](uright=uright)[1], case["kf"], case["Tcw"], case["log_sf"], th, orb_dist, ori)
    print(f"reloc_search {tag} th {th} ORBdist {orb_dist} ori {ori} uright {uright}: n {r['n']} {r['stats']}")
    assert r["n"] >= min_n
    check_against_ref(f"{tag} non-resident", g, r, gh)
    check_against_ref(f"{tag} resident", t, r, th_, with_best=False)
    return r


@pytest.mark.parametrize("uright", [True, False])
@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("th,orb_dist", [(10, 100), (3, 64)])
def test_random_frame(ctx, tf, th, orb_dist, ori, uright):
    """rectified-stereo view (with mvuRight, which the search never looks at) and mono view"""
    check_case(ctx, tf, P320, rc.random_case(P320), th, orb_dist, ori, uright, min_n=100)


@pytest.mark.parametrize("name", ["pinhole:640x480:1000:3", "kb8mono"])
def test_other_random_frames(ctx, tf, name):
    check_case(ctx, tf, name, rc.random_case(name), 10, 100, True, False, min_n=100)


def test_inputs_exercise_the_sequential_part():
    """non-vacuity, on the restatement's side, for the random cases of this file at full pyramids; a pyramid of fewer than six
    levels (test_shifted_bounds_and_other_pyramids) cannot predict six: all of its levels must occur"""
    for name, th, orb_dist in [(P320, 10, 100), (P320, 3, 64), ("pinhole:640x480:1000:3", 10, 100), ("kb8mono", 10, 100), ("kb8two", 10, 100)] + \
                              [(f"geometry:{b}:{f}:{n}", 10, 100) for b, f, n in GEOMETRY]:
        case = rc.random_case(name)
        r = rc.expected(case, th, orb_dist)
        st = r["stats"]
        print("reloc_search non-vacuity:", name, th, orb_dist, "n", r["n"], st)
        assert st["changed_by_locks"] >= 50 and st["locked_before"] > 0 and st["removed_by_histogram"] >= 3 and r["n"] >= 100, name
        assert len(st["levels"]) >= min(6, len(case["fr"]["sf"])), name


def test_relocalisation_chain_on_a_resident_frame(ctx, tf):
    """Tracking::Relocalization: (10, 100), sFound rebuilt from the frame (src/Tracking.cc:3932-3938), (3, 64) - the resident
    holder_obs carries the first call's writes into the second; then Tracking::SearchLocalPoints on what both left behind"""
    case = rc.random_case("geometry:tight:1.2:8")
    gc = sc.geometry_case("tight", 1.2, 8)
    kf, fr = case["kf"], case["fr"]
    r1 = rc.expected(case, 10, 100)
    found = np.zeros(len(kf["valid"]), bool)
    found[r1["assign"][r1["assign"] >= 0]] = True
    kf2 = dict(kf, valid=(kf["valid"].astype(bool) & ~found).astype(np.uint8))
    r2 = rc.expected(case, 3, 64, True, kf=kf2, holder=r1["holder_obs"], tag="second")
    assert r1["n"] >= 100 and r2["n"] >= 10 and (r2["holder_obs"] != r1["holder_obs"]).sum() == r2["n"]
    oF, gF = case["view"]()
    oF.holder_obs[:] = r2["holder_obs"]
    ofr = ob.is_in_frustum(oF, ob.make_pose(gc["Rcw"], gc["tcw"]), gc["pts"], 0.5, fr["log_sf"])
    o3 = ob.search_local_points(oF, sc.local_points_from_frustum(ofr, gc["pts"]), 3.0)
    tf.upload(gF)
    t1 = tf.search_keyframe_projection(kf, se3(case["Tcw"]), case["log_sf"], 10, 100)
    check_against_ref("first", t1, r1, tf.holder_obs(), with_best=False)
    found_t = np.zeros(len(kf["valid"]), bool)
    found_t[t1["assign"][t1["assign"] >= 0]] = True
    t2 = tf.search_keyframe_projection(dict(kf, valid=(kf["valid"].astype(bool) & ~found_t).astype(np.uint8)), se3(case["Tcw"]),
                                       case["log_sf"], 3, 64)
    check_against_ref("second", t2, r2, tf.holder_obs(), with_best=False)
    t3 = tf.track_local_map(orb.make_pose(gc["Rcw"], gc["tcw"]), gc["pts"], 0.5, fr["log_sf"], 3.0)
    print(f"reloc_search chain: n {r1['n']}, {r2['n']}, local map {o3['n']}")
    assert o3["n"] > 20
    assert t3["n"] == o3["n"] and np.array_equal(t3["assign"], o3["assign"]) and np.array_equal(tf.holder_obs(), oF.holder_obs)


def test_two_camera_frame_matches_left_keypoints_only(ctx, tf):
    case = rc.random_case("kb8two")
    r = check_case(ctx, tf, "kb8two", case, 10, 100, True, min_n=100)
    nleft = len(case["fr"]["kL"])
    assert case["view"](device=False)[0].Nleft == nleft and (case["holder"][nleft:] != -1).sum() > 10
    assert (r["assign"][nleft:] == -1).all() and np.array_equal(r["holder_obs"][nleft:], case["holder"][nleft:])


@pytest.mark.parametrize("bounds,factor,nlevels", GEOMETRY)
def test_shifted_bounds_and_other_pyramids(ctx, tf, bounds, factor, nlevels):
    """fractional mnMinX / mnMinY, keypoints outside the grid (tight), pyramids of 1, 2, 5, 8 and 12 levels"""
    case = rc.random_case(f"geometry:{bounds}:{factor}:{nlevels}")
    check_case(ctx, tf, f"{bounds} {factor} {nlevels}", case, 10, 100, True, min_n=100)
    if bounds == "tight":
        assert sc.grid_cells(case["fr"]["kL"], case["bounds"])[2].sum() > 10


@pytest.mark.parametrize("name", sorted(rc.hand_cases()))
def test_hand_built_case(ctx, tf, name):
    case = rc.hand_cases()[name]
    r = rc.run_hand_case(case)
    gF_of = lambda: rc.hand_view(case["keys"], case["desc"], np.array(case["holder"], np.int32), device=True)[1]
    g, gh, t, th_ = run_both(ctx, tf, gF_of, case["kf"], ob.SE3(*rc.IDENTITY), rc.LOG_SF, case["th"], case["orb_dist"], case["check_orientation"])
    check_against_ref(name, g, r, gh)
    check_against_ref(name, t, r, th_, with_best=False)
    for k, want in case["expect"].items():   # and to the expectation written out from the reference text
        got = gh.tolist() if k == "holder_obs" else g[k] if k == "n" else g[k].tolist()
        assert got == want, (name, k, got, want)


def test_more_candidates_than_a_segment_is_a_capacity_error_with_outputs_untouched(ctx, tf):
    """documented limit (include/fasttrack_amd.h): more than 256 free keypoints of the level band in one point's window ->
    FT_ERR_CAPACITY, no output written, holder_obs unchanged (view and resident); 256 are resolved exactly"""
    cap = rc.capacity_case(300, 5)
    holder = np.array(cap["holder"], np.int32)
    holder[7] = 4
    T = orb.SE3(*rc.IDENTITY)
    gF = rc.hand_view(cap["keys"], cap["desc"], holder, device=True)[1]
    from fasttrack_amd import _capi
    import ctypes as C
    keep = {}
    K, M = orb._keyframe_points(cap["kf"], keep)
    assign, bd, bi, n = np.full(300, 77, np.int32), np.full(M, 77, np.int32), np.full(M, 77, np.int32), C.c_int(77)
    rcode = _capi.lib().ft_search_keyframe_projection(ctx._h, C.byref(gF.c), C.byref(K), C.byref(T.c), rc.LOG_SF, 10.0, 100, 1, _capi.ptr(assign),
                                                     C.byref(n), _capi.ptr(bd), _capi.ptr(bi))
    assert rcode == _capi.FT_ERR_CAPACITY
    assert (assign == 77).all() and (bd == 77).all() and (bi == 77).all() and n.value == 77 and np.array_equal(gF.holder_obs, holder)
    tf.upload(rc.hand_view(cap["keys"], cap["desc"], holder, device=True)[1])
    rcode = _capi.lib().ft_tracked_frame_search_keyframe_projection(tf._h, C.byref(K), C.byref(T.c), rc.LOG_SF, 10.0, 100, 1, _capi.ptr(assign),
                                                                   C.byref(n))
    assert rcode == _capi.FT_ERR_CAPACITY and (assign == 77).all() and n.value == 77 and np.array_equal(tf.holder_obs(), holder)
    # the frame is still usable, and the device's holder_obs is what it was: exactly 256 free candidates resolve
    holder[:44] = 2
    assert (holder == -1).sum() == 256
    oF, gF = rc.hand_view(cap["keys"], cap["desc"], holder, device=True)
    r = ref.search_by_projection(oF, cap["kf"], ob.SE3(*rc.IDENTITY), rc.LOG_SF, 10, 100)
    g, gh, t, th_ = run_both(ctx, tf, lambda: rc.hand_view(cap["keys"], cap["desc"], holder, device=True)[1], cap["kf"], ob.SE3(*rc.IDENTITY),
                             rc.LOG_SF, 10, 100, True)
    assert r["n"] == 5 and r["best_idx"].tolist() == [44, 45, 46, 47, 48]
    check_against_ref("256 candidates", g, r, gh)
    check_against_ref("256 candidates", t, r, th_, with_best=False)


def test_empty_inputs_return_without_a_launch(ctx, tf):
    case = rc.random_case(P320)
    kf, T = case["kf"], se3(case["Tcw"])
    none = {k: v[:0] for k, v in kf.items()}
    invalid = dict(kf, valid=np.zeros_like(kf["valid"]))
    empty = orb.FrameView(np.zeros(0, rc.KP), np.zeros((0, 32), np.uint8), rc.SF, (0, 0, 320, 240), cam=rc.CAM)
    ctx.reset_stats()
    for tag, F_of, k in (("no point", lambda: case["view"]()[1], none), ("no valid point", lambda: case["view"]()[1], invalid),
                         ("no keypoint", lambda: empty, kf)):
        gF = F_of()
        g = orb.KernelController.search_keyframe_projection(ctx, gF, k, T, case["log_sf"], 10, 100)
        tf.upload(F_of())
        t = tf.search_keyframe_projection(k, T, case["log_sf"], 10, 100)
        assert g["n"] == 0 and t["n"] == 0 and (g["assign"] == -1).all() and (t["assign"] == -1).all(), tag
        assert (g["best_dist"] == 256).all() and (g["best_idx"] == -1).all() and len(g["best_dist"]) == len(k["valid"]), tag
        if gF.N:
            assert np.array_equal(gF.holder_obs, case["holder"]) and np.array_equal(tf.holder_obs(), case["holder"]), tag
    assert ctx.get_stat("tracked.search_keyframe_projection.launches") == (0.0, 0)
    assert ctx.get_stat("search_keyframe_projection.launches") == (0.0, 0)


def test_launch_count_is_fixed(ctx, tf):
    """three kernels per resident call whatever the inputs hold (four for the non-resident entry and for a frame loaded under
    option search_grid = 0: the grid is built for the call)"""
    case, small = rc.random_case(P320), rc.hand_cases()["second_point_takes_the_next"]
    T = se3(case["Tcw"])
    try:
        ctx.set_kernel_timing(True)
        ctx.reset_stats()
        tf.upload(case["view"]()[1])
        tf.search_keyframe_projection(case["kf"], T, case["log_sf"], 10, 100)
        tf.search_keyframe_projection(case["kf"], T, case["log_sf"], 3, 64, False)
        tf.upload(rc.hand_view(small["keys"], small["desc"], device=True)[1])
        tf.search_keyframe_projection(small["kf"], orb.SE3(*rc.IDENTITY), rc.LOG_SF, 10, 100)
        assert ctx.get_stat("tracked.search_keyframe_projection.launches") == (9.0, 3)
        for name in ("kernel.reloc_project", "kernel.reloc_candidates", "kernel.reloc_resolve"):
            assert ctx.get_stat(name)[1] == 3, name
        orb.KernelController.search_keyframe_projection(ctx, case["view"]()[1], case["kf"], T, case["log_sf"], 10, 100)
        assert ctx.get_stat("search_keyframe_projection.launches") == (4.0, 1)
        with ctx.options(search_grid=0):
            tf.upload(case["view"]()[1])
            t = tf.search_keyframe_projection(case["kf"], T, case["log_sf"], 10, 100)
        assert ctx.get_stat("tracked.search_keyframe_projection.launches") == (13.0, 4)
        check_against_ref("search_grid 0", t, rc.expected(case, 10, 100), tf.holder_obs(), with_best=False)
    finally:
        ctx.set_kernel_timing(False)


def test_invalid_arguments(ctx, tf):
    case = rc.random_case(P320)
    gF = case["view"]()[1]
    for kw in (dict(th=0.0), dict(orb_dist=256), dict(orb_dist=-1)):
        a = dict(th=10.0, orb_dist=100)
        a.update(kw)
        with pytest.raises(orb.FastTrackError) as e:
            orb.KernelController.search_keyframe_projection(ctx, gF, case["kf"], se3(case["Tcw"]), case["log_sf"], a["th"], a["orb_dist"])
        assert e.value.status == -1
    with pytest.raises(orb.FastTrackError) as e:   # not a unit quaternion
        orb.KernelController.search_keyframe_projection(ctx, gF, case["kf"], orb.SE3([0, 0, 0, 2], [0, 0, 0]), case["log_sf"], 10, 100)
    assert e.value.status == -1
    with pytest.raises(orb.FastTrackError) as e:   # the orientation check needs the keyframe's angles
        orb.KernelController.search_keyframe_projection(ctx, gF, dict(case["kf"], angle=None), se3(case["Tcw"]), case["log_sf"], 10, 100, True)
    assert e.value.status == -1
    assert np.array_equal(gF.holder_obs, case["holder"])

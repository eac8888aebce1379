"""ORBmatcher::SearchByProjection(Frame, KeyFrame, sAlreadyFound, th, ORBdist) (reference src/ORBmatcher.cc:2087-2208): the Python
restatement the GPU tests compare against (tests/reloc_search_ref.py) pinned against the committed oracle - its last-frame
search and isInFrustum, which existing tests hold to the reference - and against hand-built cases whose expected results are
written out in tests/reloc_cases.py from the reference text; the C ABI of the two entry points without a device.

What the restatement reports on the random cases (th 10, ORBdist 100 unless stated; test_inputs_exercise_the_sequential_part
asserts the conditions):
  pinhole 320x240 seed 5   730 projected, 689 searched, 4820 locked skips (1125 locked before the call), 490 choices changed by
                           locks, 340 accepted, 46 removed by the histogram, n 294, levels 0 - 7; th 3 / ORBdist 64: 776 locked
                           skips (253 before), 201 changed, 186 accepted, 11 removed, n 175
  pinhole 640x480 seed 3   1711 projected, 1615 searched, 3877 locked skips (1060 before), 953 changed, 739 accepted, 79 removed, n 660
  KannalaBrandt8 256x256   one camera: 727 projected, 687 searched, 7971 locked skips (2328 before), 493 changed, 323 accepted,
                           54 removed, n 269
"""
import ctypes as C

import numpy as np
import pytest

from fasttrack_amd import _capi
from oracle import binding as ob
from tests import reloc_cases as rc
from tests import reloc_search_ref as ref

RANDOM = ["pinhole:320x240:500:5", "pinhole:640x480:1000:3", "kb8mono"]


def test_libm_binding_and_projection_are_the_oracles():
    """project() against the oracle through isInFrustum's proj_x / proj_y (matrix pose = identity: Pc = Pw exactly)"""
    rng = np.random.default_rng(2)
    P = np.stack([rng.uniform(-1, 1, 200), rng.uniform(-1, 1, 200), rng.uniform(1, 6, 200)], 1).astype(np.float32)
    for model, cam, size in ((0, rc.CAM, (640, 480)), (1, rc.KB8_CAM_256, (256, 256))):
        F = ob.FrameView(rc.hand_keys([(10, 10)]), rc.BASE[:1], rc.SF, (0, 0) + size, cam_model=model, cam=cam)
        pts = dict(world_pos=P, normal=np.tile(np.float32([0, 0, 1]), (200, 1)), max_distance=np.full(200, 1e3, np.float32),
                   min_distance=np.zeros(200, np.float32))
        fr = ob.is_in_frustum(F, ob.make_pose(np.eye(3), np.zeros(3)), pts, -2.0, rc.LOG_SF)
        assert fr["in_view"].sum() >= 50
        for i in np.flatnonzero(fr["in_view"]):
            u, v = ref.project(model, cam, P[i])
            assert (u, v) == (fr["proj_x"][i], fr["proj_y"][i])


@pytest.mark.parametrize("name", RANDOM)
def test_equals_the_last_frame_oracle_on_its_own_levels(name):
    """With octave = the predicted level, valid = the points searched, every Observations() 1 and no point behind the camera,
    SearchByProjection(CurrentFrame, LastFrame) with forward = backward = false on a monocular view walks the same windows
    (level - 1 .. level + 1), skips the same keypoints (held with Observations() > 0) and accepts at TH_HIGH = 100"""
    case = rc.random_case(name)
    r = rc.expected(case, 10, 100)
    assert (r["zc"][r["searched"]] > 0).all()
    kf = case["kf"]
    M = len(kf["valid"])
    oF, _ = case["view"](uright=False, device=False)
    assert oF.Nleft == -1 and oF.uright is None
    oF.holder_obs[:] = np.where(case["holder"] != -1, 1, -1)
    L = dict(valid=r["searched"].astype(np.uint8), world_pos=kf["world_pos"], descriptors=kf["descriptors"],
             observations=np.ones(M, np.int32), octave=np.maximum(r["level"], 0), angle=kf["angle"])
    o = ob.search_last_frame(oF, L, case["Tcw"], 10, False, False, True)
    assert o["n"] == r["n"]
    assert np.array_equal(o["assign"], r["assign"])
    assert np.array_equal(oF.holder_obs != -1, r["holder_obs"] != -1)


@pytest.mark.parametrize("name", RANDOM)
def test_predicted_level_and_range_test_are_is_in_frustums(name):
    case = rc.random_case(name)
    r = rc.expected(case, 10, 100)
    kf = case["kf"]
    M = len(kf["valid"])
    oF, _ = case["view"](uright=False, device=False)
    T = case["Tcw"].matrix()
    pose = ob.make_pose(T[:, :3], T[:, 3])
    pose.Ow[:] = [float(v) for v in r["Ow"]]
    pts = dict(world_pos=kf["world_pos"], normal=np.tile(np.float32([0, 0, 1]), (M, 1)), max_distance=kf["max_distance"],
               min_distance=kf["min_distance"], skip=(1 - kf["valid"]).astype(np.uint8))
    fr = ob.is_in_frustum(oF, pose, pts, -2.0, case["log_sf"])
    seen = fr["in_view"].astype(bool)
    assert np.array_equal(seen, r["searched"])
    assert np.array_equal(fr["level"][seen], r["level"][seen])


@pytest.mark.parametrize("name,th,orb_dist", [(n, 10, 100) for n in RANDOM] + [(RANDOM[0], 3, 64)])
def test_inputs_exercise_the_sequential_part(name, th, orb_dist):
    st = rc.expected(rc.random_case(name), th, orb_dist)["stats"]
    assert st["changed_by_locks"] >= 50 and st["locked_before"] > 0 and st["removed_by_histogram"] >= 3
    assert rc.expected(rc.random_case(name), th, orb_dist)["n"] >= 100 and len(st["levels"]) >= 6
    assert st["locked_skips"] > st["locked_before"] and st["projected"] > st["searched"] > st["accepted"]


def test_uright_changes_nothing():
    """mvuRight is never looked at, unlike the last-frame overload (:1880-1885)"""
    case = rc.random_case(RANDOM[0])
    r = rc.expected(case, 10, 100)
    oF, _ = case["view"](uright=True, device=False)
    assert oF.uright is not None and (oF.uright > 0).sum() > 50
    s = ref.search_by_projection(oF, case["kf"], case["Tcw"], case["log_sf"], 10, 100)
    for k in ("assign", "holder_obs", "best_dist", "best_idx"):
        assert np.array_equal(r[k], s[k])
    assert r["n"] == s["n"]


@pytest.mark.parametrize("name", sorted(rc.hand_cases()))
def test_hand_built_case(name):
    case = rc.hand_cases()[name]
    r = rc.run_hand_case(case)
    for k, want in case["expect"].items():
        got = r[k].tolist() if k != "n" else r[k]
        assert got == want, (name, k, got, want)


def test_hand_built_cases_are_what_they_claim():
    c = rc.hand_cases()
    assert rc.run_hand_case(c["behind_the_camera"])["zc"][0] < 0
    assert rc.run_hand_case(c["level_zero_band"])["level"].tolist() == [0]
    assert rc.run_hand_case(c["last_level_band"])["level"].tolist() == [7]
    oF, _ = rc.hand_view(c["tie_earlier_cell_column"]["keys"], c["tie_earlier_cell_column"]["desc"])
    assert ob.features_in_area(oF, 110.0, 100.0, 15.0, -1, 1).tolist() == [1, 0]
    st = rc.run_hand_case(c["histogram_removal_had_locked"])["stats"]
    assert st["removed_by_histogram"] == 1 and st["locked_skips"] == 1 and st["locked_before"] == 0 and st["accepted"] == 13
    # without the orientation check nothing is removed
    r = rc.run_hand_case(dict(c["histogram_removal_had_locked"], check_orientation=False))
    assert r["n"] == 13 and r["assign"][0] == 0
    cap = rc.capacity_case()
    r = rc.run_hand_case(cap)
    assert r["n"] == 5 and r["best_dist"].tolist() == [0, 1, 2, 3, 4] and r["best_idx"].tolist() == [0, 1, 2, 3, 4]


def test_entry_points_are_declared_exported_and_reject_null_arguments_without_a_device():
    names = _capi.declared_symbols()
    L = _capi.lib()
    for name in ("ft_search_keyframe_projection", "ft_tracked_frame_search_keyframe_projection"):
        assert name in names
        assert hasattr(L, name)
    n = C.c_int(7)
    assign = np.zeros(4, np.int32)
    K = _capi.KeyFramePoints()
    T = _capi.SE3()
    T.q[3] = 1.0
    F = _capi.FrameView()
    F.N, F.Nleft = 0, -1
    assert L.ft_search_keyframe_projection(None, C.byref(F), C.byref(K), C.byref(T), 0.18, 10.0, 100, 1, _capi.ptr(assign), C.byref(n),
                                           None, None) == _capi.FT_ERR_INVALID
    assert b"null" in L.ft_last_error()
    assert L.ft_tracked_frame_search_keyframe_projection(None, C.byref(K), C.byref(T), 0.18, 10.0, 100, 1, _capi.ptr(assign),
                                                         C.byref(n)) == _capi.FT_ERR_INVALID
    assert n.value == 7

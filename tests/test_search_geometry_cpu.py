"""The oracle on frame geometries other than bounds (0, 0, w, h) with the 1.2 / 8-level pyramid (no GPU needed), before the
device is compared with it (tests/test_gpu_search_geometry.py):
  a. Frame::GetFeaturesInArea restated exactly in float32 numpy equals the oracle's, element for element, on shifted bounds;
  b. the inputs of the GPU tests are not vacuous: keypoints outside the grid, populated boundary cells, projections the bounds
     test decides, octaves 8 .. 11, enough matches - asserted here, so that a changed seed fails on a CPU-only machine;
  c. the directed rotation-histogram cases (scenarios.lattice_last_frame) give their hand-computed outcomes.
Seed 31 at 640x480 / 1000 features meets every condition of b, the octave condition of (1.1, 12) included (221 keypoints with
octave >= 8; 168 of them assigned by the last-frame search, 196 by the sparse local-map search)."""
import numpy as np
import pytest

from oracle import binding as ob
from tests import scenarios as sc

COLS, ROWS = 64, 48


def features_in_area_numpy(keys, bounds, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea (Frame.cc:681-747) over Frame::AssignFeaturesToGrid (:409-440), every float operation in float32
    and left to right as the reference writes it; a cell's keypoints in index order, cells column by column."""
    f32 = np.float32
    minx, miny, maxx, maxy = [f32(v) for v in bounds]
    inv_w, inv_h = f32(COLS) / f32(maxx - minx), f32(ROWS) / f32(maxy - miny)
    cx, cy, outside = sc.grid_cells(keys, bounds)
    x, y, r = f32(x), f32(y), f32(r)
    c0 = max(0, int(np.floor(f32(f32(f32(x - minx) - r) * inv_w))))
    if c0 >= COLS:
        return np.zeros(0, np.int32)
    c1 = min(COLS - 1, int(np.ceil(f32(f32(f32(x - minx) + r) * inv_w))))
    if c1 < 0:
        return np.zeros(0, np.int32)
    r0 = max(0, int(np.floor(f32(f32(f32(y - miny) - r) * inv_h))))
    if r0 >= ROWS:
        return np.zeros(0, np.int32)
    r1 = min(ROWS - 1, int(np.ceil(f32(f32(f32(y - miny) + r) * inv_h))))
    if r1 < 0:
        return np.zeros(0, np.int32)
    m = ~outside & (cx >= c0) & (cx <= c1) & (cy >= r0) & (cy <= r1)
    if min_level > 0 or max_level >= 0:
        m &= keys["octave"] >= min_level
        if max_level >= 0:
            m &= keys["octave"] <= max_level
    m &= (np.abs(keys["x"] - x) < r) & (np.abs(keys["y"] - y) < r)
    idx = np.nonzero(m)[0]
    return idx[np.lexsort((idx, cy[idx], cx[idx]))].astype(np.int32)


@pytest.mark.parametrize("name", ["default", "loose", "tight", "edge"])
def test_features_in_area_exact_restatement(name):
    total = 0
    for fr in (sc.geometry_frame(*sc.GEOMETRY_FRAME), sc.geometry_frame(512, 512, 1500, 10, two_cameras=True)):
        w, h = fr["w"], fr["h"]
        bounds = sc.frame_bounds(w, h) if name == "default" else sc.GEOMETRY_BOUNDS(w, h)[name]
        oF, _ = sc.geometry_views(fr, bounds, device=False)
        x, y, r, lo, hi, right = sc.area_queries(bounds, fr["nlevels"], 200, 8)
        for q in range(200):
            rt = bool(right[q]) and fr["two_cameras"]
            o = ob.features_in_area(oF, float(x[q]), float(y[q]), float(r[q]), int(lo[q]), int(hi[q]), rt)
            mine = features_in_area_numpy(fr["kR"] if rt else fr["kL"], bounds, x[q], y[q], r[q], int(lo[q]), int(hi[q]))
            assert np.array_equal(o, mine), (name, q, rt)
            total += len(o)
    assert total > 3000


def _project(intr, R, t, P):
    X = np.asarray(P, np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    return intr["fx"] * X[:, 0] / X[:, 2] + intr["cx"], intr["fy"] * X[:, 1] / X[:, 2] + intr["cy"], X[:, 2]


def _inside(u, v, b):
    return (u >= b[0]) & (u <= b[2]) & (v >= b[1]) & (v <= b[3])


@pytest.mark.parametrize("name,factor,nlevels", sc.GEOMETRY_CASES)
def test_geometry_cases_are_not_vacuous(name, factor, nlevels):
    c = sc.geometry_case(name, factor, nlevels)
    fr, bounds, keys = c["fr"], c["bounds"], c["fr"]["kL"]
    w, h = fr["w"], fr["h"]
    assert keys["octave"].min() == 0 and keys["octave"].max() == nlevels - 1
    cx, cy, outside = sc.grid_cells(keys, bounds)
    oF, _ = sc.geometry_views(fr, bounds, device=False)
    o1 = ob.search_last_frame(oF, c["last"], c["Tcw"], 15.0, False, False, True)
    assigned = {}
    for kind in ("dense", "sparse"):
        oF, _ = sc.geometry_views(fr, bounds, device=False)
        assigned[kind] = ob.search_local_points(oF, c["local"][kind], 7.0)
    o2 = assigned["dense"]
    few = nlevels == 1
    assert o2["n"] >= (100 if few else 150) and o1["n"] >= (150 if few else 200), (o2["n"], o1["n"])
    # the bounds test decides: projections inside the bounds and outside the image, or the other way round
    img = sc.frame_bounds(w, h)
    for what, (u, v, z) in (("last", _project(fr["intr"], c["Tcw"][:, :3], c["Tcw"][:, 3], c["last"]["world_pos"])),
                            ("frustum", _project(fr["intr"], c["Rcw"], c["tcw"], c["pts"]["world_pos"]))):
        decided = (z > 0) & (_inside(u, v, bounds) != _inside(u, v, img))
        if name in ("loose", "tight"):
            assert decided.sum() >= 20, (what, int(decided.sum()))
            one_way = _inside(u, v, bounds) & ~_inside(u, v, img) if name == "loose" else _inside(u, v, img) & ~_inside(u, v, bounds)
            assert (decided & one_way).sum() >= 20, what
    if name == "tight":
        assert outside.sum() >= 50
        ok = ~outside
        for n_cell in ((cx[ok] == 0).sum(), (cx[ok] == COLS - 1).sum(), (cy[ok] == 0).sum(), (cy[ok] == ROWS - 1).sum()):
            assert n_cell >= 3
        for o in (o1, assigned["dense"], assigned["sparse"]):
            assert (o["assign"][outside] < 0).all()
    if name == "loose":
        assert not outside.any()
    if nlevels == 12:
        high = keys["octave"] >= 8
        assert high.sum() >= 30
        # (the dense set sits on the first sixth of the keypoints - octaves 0 and 1: the sparse set is the one that reaches the top)
        assert (o1["assign"][high] >= 0).sum() >= 10 and (assigned["sparse"]["assign"][high] >= 0).sum() >= 10


def test_two_camera_frame_has_right_keypoints_outside_the_grid():
    fr = sc.geometry_frame(512, 512, 1500, 10, two_cameras=True)
    bounds = sc.GEOMETRY_BOUNDS(512, 512)["tight"]
    assert sc.grid_cells(fr["kL"], bounds)[2].sum() >= 20 and sc.grid_cells(fr["kR"], bounds)[2].sum() >= 20


# ---- c. the rotation-consistency filter, directed -----------------------------------------------------------------------------
# spec, doubles, bins that survive ComputeThreeMaxima, return value with the orientation check
DOUBLES = [(0, 9), (9, 0), (9, 9), (0, 3)]
ROTATION_CASES = {
    "third_dropped": ({0: 100, 3: 10, 7: 9, 9: 5}, (), {0, 3}, 110),          # 9 < 0.1f * 100: third maximum dropped, 10 kept
    "second_and_third_dropped": ({0: 101, 3: 10, 7: 9, 9: 5}, (), {0}, 101),   # 10 < 0.1f * 101 = 10.1
    "four_way_tie": ({2: 50, 5: 50, 8: 50, 11: 50}, (), {2, 5, 8}, 150),       # strict > : the first three in index order
    # histogram 0: 103, 3: 41, 7: 30, 9: 9 writes; bin 9 removed: 183 - 9 writes = 174 while 171 keypoints hold a point
    "doubles": ({0: 100, 3: 40, 7: 30, 9: 5}, DOUBLES, {0, 3, 7}, 174),
    "one_bin": ({4: 120}, (), {4}, 120),
    "no_point": ({}, (), set(), 0),
    "two_bins": ({1: 60, 6: 7}, (), {1, 6}, 67),
    "two_bins_second_dropped": ({1: 60, 6: 5}, (), {1}, 60),
    # -0.01 degrees: rot < 0 -> + 360 = 359.99 -> round(11.9997) = bin 12 (HISTO_LENGTH is 30: 12 is never folded onto 0)
    "wrap": ({-0.01 / 30: 40, 359.99 / 30: 30, 0: 80, 6: 20, 3: 10}, (), {12, 0, 6}, 170),
}


def rotation_expectation(lat, kept, check_orientation):
    """assign / holder_obs / n from the hand-listed surviving bins: a keypoint survives if every write to it fell into a kept bin
    (a removed write clears the keypoint whichever write came last); n counts writes, not keypoints"""
    last, kp = lat["last"], lat["kp_of_point"]
    bins = np.round(np.mod(lat["last"]["angle"].astype(np.float64), 360.0) / 30.0).astype(int)   # keypoint angles are 0
    n = len(lat["keys"])
    assign, holder = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for i in range(len(kp)):
        assign[kp[i]], holder[kp[i]] = i, last["observations"][i]
    writes = len(kp)
    if check_orientation:
        for i in range(len(kp)):
            if bins[i] not in kept:
                assign[kp[i]] = holder[kp[i]] = -1
                writes -= 1
    return assign, holder, writes


@pytest.mark.parametrize("case", list(ROTATION_CASES))
@pytest.mark.parametrize("shifted", [False, True])
def test_rotation_filter_directed_cases(case, shifted):
    spec, doubles, kept, n = ROTATION_CASES[case]
    lat = sc.lattice_last_frame(spec, doubles, bounds=sc.LATTICE_SHIFTED_BOUNDS if shifted else None)
    if shifted:   # the lattice's first column / row in grid column / row 0, its last ones short of the far border
        cx, cy, outside = sc.grid_cells(lat["keys"], lat["bounds"])
        assert not outside.any() and (cx[:1] == 0).all() and (cy[:1] == 0).all() and (cx == 0).sum() == 17
    for ori in (True, False):
        oF, _ = sc.lattice_views(lat, device=False)
        o = ob.search_last_frame(oF, lat["last"], lat["Tcw"], 2.0, False, False, ori)
        assign, holder, writes = rotation_expectation(lat, kept, ori)
        assert o["n"] == writes == (n if ori else len(lat["kp_of_point"])), (case, ori)
        assert np.array_equal(o["assign"], assign) and np.array_equal(oF.holder_obs, holder), (case, ori)
        assert np.array_equal(o["best_idx"], lat["kp_of_point"]) and (o["best_dist"] == 0).all()
    if case == "doubles":
        first = len(lat["kp_of_point"]) - 2 * len(doubles)
        dk = lat["kp_of_point"][first::2]
        assign, holder, _ = rotation_expectation(lat, kept, True)
        assert (assign[dk[:3]] == -1).all() and (holder[dk[:3]] == -1).all() and assign[dk[3]] == first + 7
        assert (assign >= 0).sum() == 171


def test_rotation_filter_nothing_accepted():
    lat = sc.lattice_last_frame({0: 50, 5: 50}, unmatched=True)
    oF, _ = sc.lattice_views(lat, device=False)
    o = ob.search_last_frame(oF, lat["last"], lat["Tcw"], 2.0, False, False, True)
    assert o["n"] == 0 and (o["assign"] == -1).all() and (o["best_dist"] == 256).all() and (oF.holder_obs == -1).all()

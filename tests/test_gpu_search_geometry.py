"""-m gpu: the tracking-side kernels on frame geometries the rest of the suite never builds - image bounds other than (0, 0, w, h)
(fractional mnMinX / mnMinY, keypoints that never enter the 64x48 grid, populated boundary cells, projections the bounds test
decides), pyramids of 1 to 12 levels with factors 1.1 to 2.0 (octaves 8 .. 11, other slab counts, another log scale factor) - and
the rotation-consistency filter of SearchByProjection(CurrentFrame, LastFrame) driven on purpose (scenarios.lattice_last_frame).
Everything is compared with the oracle for equality; tests/test_search_geometry_cpu.py pins the oracle on the same inputs and
asserts that they are not vacuous."""
import numpy as np
import pytest

from fasttrack_amd import orb
from oracle import binding as ob
from tests import init_search_ref as ref
from tests import scenarios as sc
from tests.test_search_geometry_cpu import ROTATION_CASES

pytestmark = pytest.mark.gpu

RAW = ("best_dist", "best_dist2", "best_level", "best_level2", "best_idx")
RAW_R = tuple(k + "_r" for k in RAW)
CASES = pytest.mark.parametrize("name,factor,nlevels", sc.GEOMETRY_CASES)
BATCH_OPTS = [dict(search_cache=0), dict(search_grid=0), dict(search_cache=1), dict(search_cache=1, pass_burst=2),
              dict(search_cache=0, pass_burst=2), dict(search_cache=3), dict(search_cache=2, pass_burst=2)]


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def _bounds(name, w, h):
    return sc.frame_bounds(w, h) if name == "default" else sc.GEOMETRY_BOUNDS(w, h)[name]


def _kb8(factor=1.2, nlevels=8, seed=10):
    return sc.geometry_frame(512, 512, 1500, seed, factor, nlevels, two_cameras=True)


@CASES
def test_features_in_area(ctx, name, factor, nlevels):
    total = 0
    for fr in (sc.geometry_case(name, factor, nlevels)["fr"], _kb8(factor, nlevels)):
        bounds = _bounds(name, fr["w"], fr["h"])
        oF, gF = sc.geometry_views(fr, bounds)
        x, y, r, lo, hi, right = sc.area_queries(bounds, nlevels, 300, 8)
        if not fr["two_cameras"]:
            right[:] = 0
        got, cnt = orb.features_in_area(ctx, gF, x, y, r, lo, hi, right, capacity=2048)
        for q in range(300):
            o = ob.features_in_area(oF, float(x[q]), float(y[q]), float(r[q]), int(lo[q]), int(hi[q]), bool(right[q]))
            assert cnt[q] == len(o) and np.array_equal(got[q], o), (fr["two_cameras"], q)
            total += len(o)
    assert total > 3000


@CASES
def test_search_local_points(ctx, name, factor, nlevels):
    """launchSearchLocalPointsKernel, stereo (mvuRight test) and mono, dense windows at th 1, 7 and 60, and the sparse set - the
    one that reaches every octave - at th 7; some keypoints held before the call"""
    c = sc.geometry_case(name, factor, nlevels)
    fr = c["fr"]
    rng = np.random.default_rng(5)
    holder = np.where(rng.random(len(fr["kL"])) < 0.1, rng.integers(0, 3, len(fr["kL"])), -1).astype(np.int32)
    for kind, th in (("dense", 1.0), ("dense", 7.0), ("dense", 60.0), ("mono", 1.0), ("mono", 7.0), ("mono", 60.0), ("sparse", 7.0)):
        oF, gF = sc.geometry_views(fr, c["bounds"], uright=kind != "mono", holder=holder)
        o = ob.search_local_points(oF, c["local"][kind], th)
        g = orb.KernelController.launchSearchLocalPointsKernel(ctx, gF, c["local"][kind], th)
        assert o["n"] > 50, (kind, th)
        assert g["n"] == o["n"] and np.array_equal(g["assign"], o["assign"]), (kind, th)
        assert np.array_equal(gF.holder_obs, oF.holder_obs), (kind, th)
        for k in RAW:
            assert np.array_equal(g[k], o[k]), (kind, th, k)


@CASES
def test_search_last_frame(ctx, name, factor, nlevels):
    """launchPoseEstimationKernel with the pose as a matrix and in the Sophus form: forward, backward, neither, with and without
    the orientation check"""
    c = sc.geometry_case(name, factor, nlevels)
    fr = c["fr"]
    q, t = sc.random_se3(np.random.default_rng(7), 0.03, 0.006)
    for th, fwd, bwd, ori, se3 in ((7.0, False, False, True, False), (15.0, True, False, True, False), (15.0, False, True, True, True),
                                   (7.0, False, False, False, True), (15.0, False, False, True, True), (15.0, False, False, False, False)):
        oF, gF = sc.geometry_views(fr, c["bounds"])
        oT, gT = (ob.SE3(q, t), orb.SE3(q, t)) if se3 else (c["Tcw"], c["Tcw"])
        o = ob.search_last_frame(oF, c["last"], oT, th, fwd, bwd, ori)
        g = orb.KernelController.launchPoseEstimationKernel(ctx, gF, c["last"], gT, th, fwd, bwd, ori)
        tag = (th, fwd, bwd, ori, se3)
        assert o["n"] > 50, tag
        assert g["n"] == o["n"] and np.array_equal(g["assign"], o["assign"]), tag
        assert np.array_equal(g["best_dist"], o["best_dist"]) and np.array_equal(g["best_idx"], o["best_idx"]), tag
        assert np.array_equal(gF.holder_obs, oF.holder_obs), tag


@CASES
def test_is_in_frustum(ctx, name, factor, nlevels):
    c = sc.geometry_case(name, factor, nlevels)
    fr = c["fr"]
    oF, gF = sc.geometry_views(fr, c["bounds"])
    for limit in (0.5, 0.9):
        o = ob.is_in_frustum(oF, ob.make_pose(c["Rcw"], c["tcw"]), c["pts"], limit, fr["log_sf"])
        g = orb.is_in_frustum(ctx, gF, orb.make_pose(c["Rcw"], c["tcw"]), c["pts"], limit, fr["log_sf"])
        assert 200 < o["n"] < len(c["pts"]["world_pos"]) - 200
        assert g["n"] == o["n"]
        for k, _ in ob.FRUSTUM_FIELDS:
            assert np.array_equal(g[k], o[k]), (limit, k)
    if nlevels > 1:
        assert len(np.unique(o["level"][o["in_view"] > 0])) >= min(nlevels, 4)   # PredictScale spreads over the pyramid


def _oracle_sequence(fr, bounds, c, th_last, th_local, far=False, th_far=0.0, tlr=(0, 0, 0), holder=None):
    """TrackWithMotionModel's search, isInFrustum and SearchLocalPoints on one oracle view (holder_obs carries over)"""
    oF, _ = sc.geometry_views(fr, bounds, holder=holder, device=False)
    o1 = ob.search_last_frame(oF, c["last"], c["Tcw"], th_last, False, False, True)
    ofr = ob.is_in_frustum(oF, ob.make_pose(c["Rcw"], c["tcw"], tlr), c["pts"], 0.5, fr["log_sf"])
    o2 = ob.search_local_points(oF, sc.local_points_from_frustum(ofr, c["pts"], far, th_far), th_local)
    return o1, ofr, o2, oF.holder_obs.copy()


def _check_sequence(tag, g1, g2, gh, o1, ofr, o2, oh):
    assert g1["n"] == o1["n"] and np.array_equal(g1["assign"], o1["assign"]), f"{tag}: last-frame search"
    for k, _ in ob.FRUSTUM_FIELDS:
        assert np.array_equal(g2[k], ofr[k]), f"{tag}: frustum field {k}"
    assert g2["n_to_match"] == ofr["n"], f"{tag}: nToMatch"
    assert g2["n"] == o2["n"] and np.array_equal(g2["assign"], o2["assign"]), f"{tag}: local-map search"
    assert np.array_equal(gh, oh), f"{tag}: holder_obs"


@CASES
def test_tracked_frame_sequence(ctx, name, factor, nlevels):
    """the sequence of test_tracked_frame_sequence_equals_oracle on the resident frame, with and without far-point rejection"""
    c = sc.geometry_case(name, factor, nlevels)
    fr = c["fr"]
    depth = fr["sm"]["depth"]
    tf = orb.TrackedFrame(ctx, max_keypoints=4096, max_points=4096)
    try:
        for far in (False, True):
            th_far = float(np.percentile(depth[depth > 0], 85)) if far else 0.0
            o1, ofr, o2, oh = _oracle_sequence(fr, c["bounds"], c, 15.0, 3.0, far, th_far)
            _, gF = sc.geometry_views(fr, c["bounds"])
            tf.upload(gF)
            g1 = tf.search_last_frame(c["last"], c["Tcw"], 15.0)
            g2 = tf.track_local_map(orb.make_pose(c["Rcw"], c["tcw"]), c["pts"], 0.5, fr["log_sf"], 3.0, far_points=far, th_far_points=th_far)
            # (one level: 548 keypoints, 358 of them held by the first search already - the second finds about 20 free ones)
            assert o1["n"] > 100 and o2["n"] > (10 if nlevels == 1 else 30)
            _check_sequence(f"far {far}", g1, g2, tf.holder_obs(), o1, ofr, o2, oh)
    finally:
        tf.close()


def _kb8_case(fr, seed):
    last, Tcw, pts, Rcw, tcw, tlr = sc.geometry_inputs(fr, seed, M=1500)
    return dict(last=last, Tcw=Tcw, pts=pts, Rcw=Rcw, tcw=tcw)


def test_two_camera_kb8_frame_with_tight_bounds(ctx):
    """local-map search, last-frame search (KannalaBrandt8 projection, right camera through Trl) and isInFrustum on a two-camera frame
    whose left AND right keypoints partly lie outside the grid"""
    fr = _kb8()
    bounds = _bounds("tight", 512, 512)
    NL = len(fr["kL"])
    outL, outR = sc.grid_cells(fr["kL"], bounds)[2], sc.grid_cells(fr["kR"], bounds)[2]
    assert outL.sum() >= 20 and outR.sum() >= 20
    outside = np.concatenate([outL, outR])
    pts = sc.two_camera_points(fr, fr["sf"], 3)
    for th in (1.0, 7.0):
        oF, gF = sc.geometry_views(fr, bounds)
        o = ob.search_local_points(oF, pts, th)
        g = orb.KernelController.launchSearchLocalPointsKernel(ctx, gF, pts, th)
        assert o["n"] > 50 and (o["assign"][NL:] >= 0).sum() > 10
        assert g["n"] == o["n"] and np.array_equal(g["assign"], o["assign"]) and np.array_equal(gF.holder_obs, oF.holder_obs)
        for k in RAW + RAW_R:
            assert np.array_equal(g[k], o[k]), (th, k)
    c = _kb8_case(fr, 4)
    oF, gF = sc.geometry_views(fr, bounds)
    o = ob.search_last_frame(oF, c["last"], c["Tcw"], 15.0, False, False, True)
    g = orb.KernelController.launchPoseEstimationKernel(ctx, gF, c["last"], c["Tcw"], 15.0, False, False, True)
    assert o["n"] > 30 and (o["best_idx_r"] >= 0).sum() > 30
    assert g["n"] == o["n"] and np.array_equal(g["assign"], o["assign"]) and np.array_equal(gF.holder_obs, oF.holder_obs)
    for k in ("best_dist", "best_idx", "best_dist_r", "best_idx_r"):
        assert np.array_equal(g[k], o[k]), k
    # a keypoint outside the grid is matched by the left <-> right table alone (never by a window): the oracle's own count
    assert (o["assign"][outside] >= 0).sum() < outside.sum() // 2
    oF, gF = sc.geometry_views(fr, bounds)
    ofr = ob.is_in_frustum(oF, ob.make_pose(c["Rcw"], c["tcw"], sc.KB8_TLR), c["pts"], 0.5, fr["log_sf"])
    gfr = orb.is_in_frustum(ctx, gF, orb.make_pose(c["Rcw"], c["tcw"], sc.KB8_TLR), c["pts"], 0.5, fr["log_sf"])
    assert ofr["in_view"].sum() > 200 and ofr["in_view_r"].sum() > 200 and gfr["n"] == ofr["n"]
    for k, _ in ob.FRUSTUM_FIELDS:
        assert np.array_equal(gfr[k], ofr[k]), k


@pytest.mark.parametrize("name", ["tight", "loose"])
def test_search_for_initialization(ctx, name):
    """SearchForInitialization (windows on level 0 only) with both frames under shifted bounds: the non-resident and the resident
    entry against the restatement, compared as tests/test_gpu_init_search.py compares them"""
    from tests import test_gpu_init_search as tis
    w, h, nf, seed, dx, dy = tis.REAL[0]   # displaced by (4, 12): a window of 15 still finds it
    k1, d1, k2, d2 = tis.real_pair(ctx, w, h, nf, seed, dx, dy)
    bounds = _bounds(name, w, h)
    level0 = k2["octave"] == 0
    outside = sc.grid_cells(k2, bounds)[2]
    for window, ratio, ori in ((100, 0.9, True), (15, 0.9, False)):
        o2, g2 = ob.FrameView(k2, d2, tis.SF, bounds), orb.FrameView(k2, d2, tis.SF, bounds)
        g1 = orb.FrameView(k1, d1, tis.SF, bounds)
        o = ref.search_for_initialization(k1, d1, o2, tis.prev_of(k1), window, ratio, ori)
        g = orb.KernelController.search_for_initialization(ctx, g1, g2, tis.prev_of(k1), window, ratio, ori)
        ini, cur = orb.TrackedFrame(ctx, max(len(k1), 1), 1), orb.TrackedFrame(ctx, max(len(k2), 1), 1)
        try:
            ini.upload(g1)
            cur.upload(g2)
            t = cur.search_for_initialization(ini, tis.prev_of(k1), window, ratio, ori)
        finally:
            ini.close()
            cur.close()
        tis.check_against_ref(f"{name} non-resident", g, o)
        tis.check_against_ref(f"{name} resident", t, o, with_distance=False)
        assert o["n"] >= 100
        matched = o["matches12"][o["matches12"] >= 0]
        if name == "tight":
            assert (outside & level0).sum() >= 10 and not outside[matched].any()
        else:
            assert not outside.any()


# ---- batched ----------------------------------------------------------------------------------------------------------------------
_batch_cache = {}


def _pinhole_batch():
    """8 pinhole frames, factor 1.2: every bounds value (the default included) and 8, 5, 12 and 1 levels in one batch - one
    log_scale_factor serves a track_local_map call"""
    if "pinhole" not in _batch_cache:
        cases = []
        for f, (name, nl) in enumerate(zip(("default", "loose", "tight", "edge", "tight", "default", "edge", "loose"), (8, 5, 12, 1, 8, 12, 5, 1))):
            c = sc.geometry_case(name, 1.2, nl)
            cases.append((c, _oracle_sequence(c["fr"], c["bounds"], c, 15.0, 7.0)))
        _batch_cache["pinhole"] = cases
    return _batch_cache["pinhole"]


def _run_batch(ctx, cases, tlr, th_last, th_local, log_sf):
    views = [sc.geometry_views(c["fr"], c["bounds"])[1] for c, _ in cases]
    tb = orb.TrackedBatch(ctx, max_frames=len(cases), max_keypoints=max(F.c.N for F in views) + 8, max_points=4096)
    try:
        tb.upload(views)
        g1 = tb.search_last_frame([c["last"] for c, _ in cases], [c["Tcw"] for c, _ in cases], th_last)
        g2 = tb.track_local_map([orb.make_pose(c["Rcw"], c["tcw"], tlr) for c, _ in cases], [c["pts"] for c, _ in cases], 0.5, log_sf, th_local)
        return g1, g2, [tb.holder_obs(f) for f in range(len(cases))]
    finally:
        tb.close()


LOG_12 = float(np.float32(np.log(np.float32(1.2))))


def test_tracked_batch_every_bounds_and_four_pyramid_depths(ctx):
    cases = _pinhole_batch()
    g1, g2, gh = _run_batch(ctx, cases, (0, 0, 0), 15.0, 7.0, LOG_12)
    assert len({c["fr"]["nlevels"] for c, _ in cases}) == 4
    for f, (c, o) in enumerate(cases):
        assert o[0]["n"] > 100 and o[2]["n"] > 30
        _check_sequence(f"frame {f}", g1[f], g2[f], gh[f], *o)
    tf = orb.TrackedFrame(ctx, max_keypoints=4096, max_points=4096)   # the single-frame path on two of them
    try:
        for f in (2, 3):
            c, o = cases[f]
            tf.upload(sc.geometry_views(c["fr"], c["bounds"])[1])
            s1 = tf.search_last_frame(c["last"], c["Tcw"], 15.0)
            s2 = tf.track_local_map(orb.make_pose(c["Rcw"], c["tcw"]), c["pts"], 0.5, LOG_12, 7.0)
            _check_sequence(f"single frame {f}", s1, s2, tf.holder_obs(), *o)
    finally:
        tf.close()


@pytest.mark.parametrize("opts", BATCH_OPTS)
def test_tracked_batch_geometry_without_cache_without_grid_with_short_bursts(ctx, opts):
    """the same batch under the option sets of test_tracked_batch_without_cache_without_grid_with_short_bursts: the grid-less and
    cache-less kernels, the claim passes and the one-launch resolution see the shifted bounds and the mixed pyramids too"""
    cases = _pinhole_batch()
    with ctx.options(**opts):
        g1, g2, gh = _run_batch(ctx, cases, (0, 0, 0), 15.0, 7.0, LOG_12)
    for f, (c, o) in enumerate(cases):
        _check_sequence(f"{opts} frame {f}", g1[f], g2[f], gh[f], *o)


def test_tracked_batch_kb8_tight_and_default_bounds(ctx):
    """two-camera KannalaBrandt8 frames with tight and default bounds in one batch, two of them through the single-frame path too"""
    if "kb8" not in _batch_cache:
        cases = []
        for f in range(8):
            fr = _kb8(seed=10 + f % 2)
            c = dict(_kb8_case(fr, 20 + f), fr=fr, bounds=_bounds("tight" if f % 2 == 0 or f == 5 else "default", 512, 512))
            cases.append((c, _oracle_sequence(fr, c["bounds"], c, 15.0, 7.0, tlr=sc.KB8_TLR)))
        _batch_cache["kb8"] = cases
    cases = _batch_cache["kb8"]
    g1, g2, gh = _run_batch(ctx, cases, sc.KB8_TLR, 15.0, 7.0, LOG_12)
    for f, (c, o) in enumerate(cases):
        assert o[0]["n"] > 30 and o[2]["n"] > 30
        _check_sequence(f"frame {f}", g1[f], g2[f], gh[f], *o)
    tf = orb.TrackedFrame(ctx, max_keypoints=4096, max_points=4096)
    try:
        for f in (0, 5):
            c, o = cases[f]
            tf.upload(sc.geometry_views(c["fr"], c["bounds"])[1])
            s1 = tf.search_last_frame(c["last"], c["Tcw"], 15.0)
            s2 = tf.track_local_map(orb.make_pose(c["Rcw"], c["tcw"], sc.KB8_TLR), c["pts"], 0.5, LOG_12, 7.0)
            _check_sequence(f"single frame {f}", s1, s2, tf.holder_obs(), *o)
    finally:
        tf.close()


def test_tracked_batch_last_frame_search_with_two_pyramids_side_by_side(ctx):
    """factor 1.5 / 5 levels and factor 1.1 / 12 levels in one search_last_frame call (no log_scale_factor involved)"""
    cases = [sc.geometry_case(name, *pyr) for name, pyr in zip(("tight", "tight", "loose", "edge", "default", "loose", "edge", "default"),
                                                               [(1.5, 5), (1.1, 12)] * 4)]
    views, want = [], []
    for c in cases:
        oF, gF = sc.geometry_views(c["fr"], c["bounds"])
        want.append((ob.search_last_frame(oF, c["last"], c["Tcw"], 15.0, False, False, True), oF.holder_obs))
        views.append(gF)
    tb = orb.TrackedBatch(ctx, max_frames=8, max_keypoints=max(F.c.N for F in views) + 8, max_points=4096)
    try:
        tb.upload(views)
        g = tb.search_last_frame([c["last"] for c in cases], [c["Tcw"] for c in cases], 15.0)
        for f, (o, oh) in enumerate(want):
            assert o["n"] > 100
            assert g[f]["n"] == o["n"] and np.array_equal(g[f]["assign"], o["assign"]) and np.array_equal(tb.holder_obs(f), oh), f
    finally:
        tb.close()


# ---- the rotation-consistency filter, directed ------------------------------------------------------------------------------------
def _lattice(case, shifted):
    spec, doubles, _, _ = ROTATION_CASES[case]
    return sc.lattice_last_frame(spec, doubles, bounds=sc.LATTICE_SHIFTED_BOUNDS if shifted else None)


@pytest.mark.parametrize("case", list(ROTATION_CASES))
@pytest.mark.parametrize("shifted", [False, True])
def test_rotation_filter_one_shot_and_resident_frame(ctx, case, shifted):
    """(the outcomes themselves - which bins survive, n counting writes, the doubled keypoints - are asserted on the oracle in
    tests/test_search_geometry_cpu.py)"""
    lat = _lattice(case, shifted)
    n_expected = ROTATION_CASES[case][3]
    tf = orb.TrackedFrame(ctx, max_keypoints=len(lat["keys"]) + 8, max_points=512)
    try:
        for ori in (True, False):
            oF, gF = sc.lattice_views(lat)
            o = ob.search_last_frame(oF, lat["last"], lat["Tcw"], 2.0, False, False, ori)
            g = orb.KernelController.launchPoseEstimationKernel(ctx, gF, lat["last"], lat["Tcw"], 2.0, False, False, ori)
            assert o["n"] == (n_expected if ori else len(lat["kp_of_point"]))
            assert g["n"] == o["n"] and np.array_equal(g["assign"], o["assign"]), ori
            assert np.array_equal(g["best_dist"], o["best_dist"]) and np.array_equal(g["best_idx"], o["best_idx"]), ori
            assert np.array_equal(gF.holder_obs, oF.holder_obs), ori
            tf.upload(sc.lattice_views(lat)[1])
            t = tf.search_last_frame(lat["last"], lat["Tcw"], 2.0, False, False, ori)
            assert t["n"] == o["n"] and np.array_equal(t["assign"], o["assign"]) and np.array_equal(tf.holder_obs(), oF.holder_obs), ori
    finally:
        tf.close()


@pytest.mark.parametrize("opts", [dict(), dict(search_cache=1), dict(search_cache=3), dict(search_grid=0)])
def test_rotation_filter_all_cases_in_one_batch(ctx, opts):
    """every directed case, on default and on shifted bounds, plus a frame on which nothing is accepted, as the frames of ONE
    TrackedBatch.search_last_frame: k_replay_batch with differently shaped histograms in one launch"""
    lats = [_lattice(case, shifted) for shifted in (False, True) for case in ROTATION_CASES]
    lats.append(sc.lattice_last_frame({0: 50, 5: 50}, unmatched=True))
    with ctx.options(**opts):
        tb = orb.TrackedBatch(ctx, max_frames=len(lats), max_keypoints=len(lats[0]["keys"]) + 8, max_points=512)
        try:
            for ori in (True, False):
                want = []
                for lat in lats:
                    oF, _ = sc.lattice_views(lat, device=False)
                    want.append((ob.search_last_frame(oF, lat["last"], lat["Tcw"], 2.0, False, False, ori), oF.holder_obs))
                tb.upload([sc.lattice_views(lat)[1] for lat in lats])
                g = tb.search_last_frame([lat["last"] for lat in lats], [lat["Tcw"] for lat in lats], 2.0, check_orientation=ori)
                for f, (o, oh) in enumerate(want):
                    assert g[f]["n"] == o["n"] and np.array_equal(g[f]["assign"], o["assign"]), (opts, ori, f)
                    assert np.array_equal(tb.holder_obs(f), oh), (opts, ori, f)
                assert len({o["n"] for o, _ in want}) >= (8 if ori else 6)
        finally:
            tb.close()

"""ft_fuse_search against the restatement of ORBmatcher::Fuse (tests/fuse_ref.py, pinned on the CPU by test_fuse_cpu.py), bit for
bit: bestIdx, bestDist, the exit code of every point and the count of points with bestDist <= TH_LOW.  Needs an MI355X.

The inputs are those of tests/fuse_cases.py; the conditions they meet are asserted in test_fuse_cpu.py.  Every case holds a few
hundred keypoints and at most 2 600 points."""
import ctypes as C

import numpy as np
import pytest

from fasttrack_amd import _capi, orb
from oracle import binding as ob
from tests import fuse_cases as fc
from tests import fuse_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def same(tag, g, k, r):
    for f in ("best_idx", "best_dist", "stage"):
        bad = np.nonzero(g[f][k] != r[f])[0]
        assert len(bad) == 0, f"{tag}: {f} differs at {bad[:5].tolist()}: {g[f][k][bad[:5]].tolist()} != {r[f][bad[:5]].tolist()}"
    assert int(g["n_found"][k]) == r["n_found"], f"{tag}: n_found {g['n_found'][k]} != {r['n_found']}"


@pytest.mark.parametrize("th,check", [(3.0, True), (4.0, False)])
@pytest.mark.parametrize("name", fc.RANDOM)
def test_random_case(ctx, name, th, check):
    """th 3 with the chi-square test (the SE3 overload, Local Mapping), th 4 without (the Sim3 overload, Loop Closing)"""
    case = fc.random_case(name)
    r = fc.expected(case, th, check)
    g = orb.fuse_search(ctx, case["points"], [fc.target_of(case, case["view"]()[1], th, check)])
    print(f"fuse {name} th {th} check {check}: n_found {r['n_found']} {r['stats']}")
    assert r["n_found"] >= 50
    same(name, g, 0, r)


def three_targets():
    """kb8two's points against: its left camera (SE3 overload), its right camera (bRight, its own pose, another valid), and its first
    700 left keypoints as a one-camera keyframe (another N, the Sim3 overload at th 4, no valid)"""
    a, b = fc.random_case("kb8two"), fc.random_case("kb8two:right")
    fr = fc.rc.random_case("kb8two")["fr"]
    kw = dict(keys=fr["kL"][:700], descriptors=fr["dL"][:700], bounds=fc.sc.frame_bounds(512, 512), cam_model=1, cam=list(fc.sc.KB8_CAM))
    c = dict(a, view=lambda device=True: (ob.FrameView(scale_factors_=fr["sf"], **kw), orb.FrameView(scale_factors=fr["sf"], **kw) if device else None))
    pts = a["points"]
    specs = [(a, 3.0, True, a["valid"]), (b, 3.0, True, np.roll(a["valid"], 7)), (c, 4.0, False, None)]
    targets = [fc.target_of(case, case["view"]()[1], th, check, valid=valid) for case, th, check, valid in specs]
    refs = [ref.fuse(case["view"](device=False)[0], pts, case["Tcw"], case["Ow"], case["log_sf"], th, case["right"], case["cam2"], valid, check)
            for case, th, check, valid in specs]
    return pts, targets, refs


def test_three_targets_equal_three_calls(ctx):
    pts, targets, refs = three_targets()
    assert len({t["kf"].N for t in targets}) >= 2 and [t["right"] for t in targets] == [False, True, False]
    ctx.reset_stats()
    g = orb.fuse_search(ctx, pts, targets)
    total3, calls3 = ctx.get_stat("fuse.launches")
    for k, r in enumerate(refs):
        same(f"target {k} of 3", g, k, r)
    assert refs[0]["n_found"] >= 50 and refs[1]["n_found"] >= 1 and refs[2]["n_found"] >= 50
    ctx.reset_stats()
    for k, t in enumerate(targets):
        s = orb.fuse_search(ctx, pts, [t])
        for f in ("best_idx", "best_dist", "stage"):
            assert np.array_equal(s[f][0], g[f][k]), (k, f)
        assert s["n_found"][0] == g["n_found"][k]
    total1, calls1 = ctx.get_stat("fuse.launches")
    # the number of launches per call does not depend on the number of targets
    assert calls3 == 1 and calls1 == 3 and total3 == total1 / 3 == 2


@pytest.mark.parametrize("name", sorted(fc.hand_cases()))
def test_hand_case(ctx, name):
    case = fc.hand_cases()[name]
    r = fc.run_hand_case(case)
    _, gF = fc.hand_view(case["keys"], case["desc"], case["uright"], device=True, keys_right=case["keys_right"])
    g = orb.fuse_search(ctx, case["points"], [fc.hand_target(case, gF)])
    same(name, g, 0, r)
    for k in ("best_idx", "best_dist", "stage"):
        assert g[k][0].tolist() == case["expect"][k], (name, k)
    assert int(g["n_found"][0]) == case["expect"]["n_found"]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 130])
def test_in_band_keypoints_of_one_cell(ctx, n):
    """rounds of 16 (and of 64) entries with and without a tail; three more keypoints of another octave share the cell"""
    case = fc.cell_crowd(n)
    r = fc.run_hand_case(case)
    _, gF = fc.hand_view(case["keys"], case["desc"], device=True)
    g = orb.fuse_search(ctx, case["points"], [fc.hand_target(case, gF)])
    same(f"crowd {n}", g, 0, r)
    assert g["best_dist"][0, 0] == 1 and g["best_idx"][0, 0] == max(n // 2 - 1, 0)


@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_point_counts(ctx, M):
    case = fc.random_case(fc.RANDOM[0])
    r = fc.expected(case, 3.0, True)
    pts = {k: v[:M] for k, v in case["points"].items()}
    g = orb.fuse_search(ctx, pts, [fc.target_of(case, case["view"]()[1], 3.0, True, valid=case["valid"][:M])])
    for f in ("best_idx", "best_dist", "stage"):
        assert np.array_equal(g[f][0], r[f][:M]), f
    assert g["n_found"][0] == int((r["best_dist"][:M] <= ref.TH_LOW).sum())


def test_empty_inputs(ctx):
    case = fc.random_case(fc.RANDOM[0])
    oF, gF = case["view"]()
    M = len(case["valid"])
    # a keyframe without keypoints: every point leaves where the restatement says, none finds anything
    kw = dict(keys=np.zeros(0, ob.KP_DTYPE), descriptors=np.zeros((0, 32), np.uint8), bounds=fc.sc.frame_bounds(320, 240),
              cam=[oF.c.cam[i] for i in range(8)])
    e_o, e_g = ob.FrameView(scale_factors_=oF.sf, **kw), orb.FrameView(scale_factors=gF.sf, **kw)
    r = ref.fuse(e_o, case["points"], case["Tcw"], case["Ow"], case["log_sf"], 3.0, valid=case["valid"])
    g = orb.fuse_search(ctx, case["points"], [fc.target_of(case, e_g, 3.0, True), fc.target_of(case, gF, 3.0, True)])
    same("N == 0", g, 0, r)
    same("beside N == 0", g, 1, fc.expected(case, 3.0, True))
    assert (g["best_idx"][0] == -1).all() and (g["best_dist"][0] == 256).all() and (g["stage"][0] == ref.EMPTY).sum() >= 100
    # nothing valid
    g = orb.fuse_search(ctx, case["points"], [fc.target_of(case, gF, 3.0, True, valid=np.zeros(M, np.uint8))])
    assert (g["best_idx"] == -1).all() and (g["best_dist"] == 256).all() and (g["stage"] == ref.SKIPPED).all() and g["n_found"][0] == 0
    # no points, no targets
    none = {k: v[:0] for k, v in case["points"].items()}
    g = orb.fuse_search(ctx, none, [fc.target_of(case, gF, 3.0, True, valid=None)])
    assert g["best_idx"].shape == (1, 0) and g["n_found"].tolist() == [0]
    g = orb.fuse_search(ctx, case["points"], [])
    assert g["best_idx"].shape == (0, M) and len(g["n_found"]) == 0


@pytest.mark.parametrize("name", ["geometry:tight:1.2:1", "geometry:tight:1.1:12", "geometry:tight:1.2:8", "geometry:loose:1.2:8"])
def test_pyramids_and_shifted_bounds(ctx, name):
    """a 1-level and a 12-level pyramid; bounds with fractional mnMinX inside the image (keypoints outside the 64 x 48 grid) and
    around it"""
    case = fc.random_case(name)
    for th, check in ((3.0, True), (4.0, False)):
        r = fc.expected(case, th, check)
        g = orb.fuse_search(ctx, case["points"], [fc.target_of(case, case["view"]()[1], th, check)])
        print(f"fuse {name} th {th}: n_found {r['n_found']} {r['stats']}")
        assert r["stats"]["stages"][ref.SEARCHED] >= 20 and r["n_found"] >= 1 and r["stats"]["stages"][ref.IMAGE] >= 1
        same(f"{name} th {th}", g, 0, r)


def test_stage_may_be_null(ctx):
    case = fc.random_case("kb8mono")
    r = fc.expected(case, 3.0, True)
    g = orb.fuse_search(ctx, case["points"], [fc.target_of(case, case["view"]()[1], 3.0, True)], want_stage=False)
    assert g["stage"] is None
    assert np.array_equal(g["best_idx"][0], r["best_idx"]) and np.array_equal(g["best_dist"][0], r["best_dist"]) and g["n_found"][0] == r["n_found"]


def test_invalid_arguments(ctx):
    case = fc.random_case(fc.RANDOM[0])

    def bad(points, target):
        with pytest.raises(orb.FastTrackError) as e:
            orb.fuse_search(ctx, points, [target])
        assert e.value.status == _capi.FT_ERR_INVALID

    _, gF = case["view"]()
    bad(case["points"], dict(fc.target_of(case, gF, 3.0, True), right=True, cam2=[1.0] * 8))     # right on a view with Nleft == -1
    _, gF = case["view"]()
    gF.c.cam_model = 7
    bad(case["points"], fc.target_of(case, gF, 3.0, True))                                        # an unknown camera model
    hand = fc.hand_cases()["right_adds_nleft"]                                                    # a keypoint octave outside [0, nlevels)
    for kl, kr, right in (([0, 8], [0, 0], False), ([0, 0], [0, -1], True)):
        _, hF = fc.hand_view(fc.hand_keys([(300, 220), (10, 10)], octave=kl), hand["desc"], device=True,
                             keys_right=fc.hand_keys([(50, 50), (300, 220)], octave=kr))
        bad(hand["points"], fc.hand_target(dict(hand, right=right), hF))
    _, gF = case["view"]()
    bad(case["points"], dict(fc.target_of(case, gF, 3.0, True), th=0.0))
    q = orb.SE3([0, 0, 0, 2], [0, 0, 0])
    bad(case["points"], dict(fc.target_of(case, gF, 3.0, True), Tcw=q))                           # not a unit quaternion
    # null arrays: the points' normals, the outputs
    M = len(case["valid"])
    keep = {k: np.ascontiguousarray(v) for k, v in case["points"].items()}
    P = _capi.FusePoints()
    P.M = M
    P.world_pos, P.normal = _capi.ptr(keep["world_pos"]), None
    P.max_distance, P.min_distance, P.descriptors = _capi.ptr(keep["max_distance"]), _capi.ptr(keep["min_distance"]), _capi.ptr(keep["descriptors"])
    T = (_capi.FuseTarget * 1)()
    T[0].kf = C.pointer(gF.c)
    T[0].Tcw = orb.SE3(case["Tcw"].q, case["Tcw"].t).c
    T[0].th, T[0].log_scale_factor = 3.0, case["log_sf"]
    T[0].Ow[:] = [float(v) for v in case["Ow"]]
    bi, bd, nf = np.full(M, 7, np.int32), np.full(M, 7, np.int32), np.full(1, 7, np.int32)
    L = _capi.lib()
    assert L.ft_fuse_search(ctx._h, C.byref(P), 1, T, _capi.ptr(bi), _capi.ptr(bd), None, _capi.ptr(nf)) == _capi.FT_ERR_INVALID
    P.normal = _capi.ptr(keep["normal"])
    assert L.ft_fuse_search(ctx._h, C.byref(P), 1, T, None, _capi.ptr(bd), None, _capi.ptr(nf)) == _capi.FT_ERR_INVALID
    assert L.ft_fuse_search(ctx._h, C.byref(P), 1, None, _capi.ptr(bi), _capi.ptr(bd), None, _capi.ptr(nf)) == _capi.FT_ERR_INVALID
    assert (bi == 7).all() and (bd == 7).all() and nf[0] == 7
    assert L.ft_fuse_search(ctx._h, C.byref(P), 1, T, _capi.ptr(bi), _capi.ptr(bd), None, _capi.ptr(nf)) == 0   # and the same call complete
    assert np.array_equal(bd, orb.fuse_search(ctx, case["points"], [fc.target_of(case, gF, 3.0, False, valid=None)])["best_dist"][0])

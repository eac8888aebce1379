"""Inputs of the SearchByProjection(KeyFrame, Sim3) tests (test_sim3_search_cpu.py, test_gpu_sim3_search.py): seeded random cases on
the frames of reloc_cases.random_case and hand-built cases of a few keypoints, each with the restatement's result
(tests/sim3_search_ref.py) computed once and shared.

A random case: reloc_cases' keyframe points (every keypoint once, then as many repeats moved by 1 cm) plus half as many more repeats -
two to three points per keypoint - with 0 .. 6 bits of every descriptor flipped, so that several points want the same keypoint and
most of them are within the threshold; normals, the reflected and the shifted twentieths as fuse_cases.fuse_points; a dozen points
aimed at places without a keypoint within 12 pixels (an empty window at level 0); 85 % valid; 20 % of the keypoints held on entry.
"""
import numpy as np

from oracle import binding as ob
from tests import fuse_cases as fc
from tests import reloc_cases as rc
from tests import reloc_search_ref as rref
from tests import sim3_search_ref as ref

RANDOM = ["pinhole:320x240:500:5", "pinhole:640x480:900:3", "kb8mono", "kb8two"]
GEOMETRY = [("loose", 1.2, 8), ("tight", 1.2, 8), ("edge", 1.2, 8), ("tight", 1.2, 1), ("tight", 2.0, 2), ("tight", 1.5, 5), ("tight", 1.1, 12)]
PARAMS = [(8, 1.5), (5, 1.0), (3, 1.5)]   # LoopClosing.cc:755 / :964, :777, and the tightest window with the wide threshold
# the (case, th, ratio, hand_pinhole) the GPU tests run: both forms at every parameter pair on the first case, the :755 and :777
# calls on the other cameras, the :755 call on the shifted bounds and the other pyramids
USED = [(RANDOM[0], th, ratio, hand) for th, ratio in PARAMS for hand in (False, True)] + \
       [(name, th, ratio, hand) for name in RANDOM[1:] for th, ratio, hand in ((8, 1.5, True), (5, 1.0, False))] + \
       [(f"geometry:{b}:{f}:{n}", 8, 1.5, True) for b, f, n in GEOMETRY]
HELD = 1 << 20                           # what a keypoint held on entry reads (any value but -1)
_cases = {}


def _rotation(q):
    x, y, z, w = [float(c) for c in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def lonely_points(oF, Tcw, n, seed):
    """n points of level 0 that project where no left keypoint lies within 12 pixels -> (world [n, 3], max_distance [n])"""
    rng = np.random.default_rng(seed + 4000)
    nleft = oF.c.N if oF.Nleft == -1 else oF.Nleft
    kx, ky = oF.keys["x"][:nleft].astype(np.float64), oF.keys["y"][:nleft].astype(np.float64)
    cam = [oF.c.cam[i] for i in range(8)]
    R, t = _rotation(Tcw.q), np.asarray(Tcw.t, np.float64)
    out = []
    for _ in range(20000):
        if len(out) == n:
            break
        u = rng.uniform(oF.c.mnMinX + 2, oF.c.mnMaxX - 2)
        v = rng.uniform(oF.c.mnMinY + 2, oF.c.mnMaxY - 2)
        if nleft and np.min(np.maximum(np.abs(kx - u), np.abs(ky - v))) < 12:
            continue
        if oF.c.cam_model == 1:
            rx, ry = rc.kb8_unproject(cam, np.array([u]), np.array([v]))
            rx, ry = float(rx[0]), float(ry[0])
        else:
            rx, ry = (u - cam[2]) / cam[0], (v - cam[3]) / cam[1]
        z = rng.uniform(2.0, 6.0)
        out.append(R.T @ (np.array([rx * z, ry * z, z]) - t))
    assert len(out) == n, "no place without keypoints in this frame"
    return np.array(out, np.float32)


def sim3_points(base, seed):
    """-> (points dict, valid, Ow, matched on entry)"""
    rng = np.random.default_rng(seed + 5000)
    kf, Tcw = base["kf"], base["Tcw"]
    oF, _ = base["view"](device=False)
    M0 = len(kf["world_pos"])
    extra = rng.integers(0, M0, M0 // 2)
    src = np.concatenate([np.arange(M0), extra])
    world = np.concatenate([kf["world_pos"], kf["world_pos"][extra] + rng.normal(0, 0.01, (len(extra), 3))]).astype(np.float32)
    desc = kf["descriptors"][src].copy()
    for i in range(len(desc)):
        desc[i] = rc.flip(desc[i], rng.choice(256, rng.integers(0, 7), replace=False))
    grown = dict(world_pos=world, max_distance=kf["max_distance"][src], min_distance=kf["min_distance"][src], descriptors=desc,
                 valid=(rng.random(len(src)) < 0.85).astype(np.uint8))
    pts, valid, Ow = fc.fuse_points(grown, Tcw, seed)
    lone = lonely_points(oF, Tcw, 12, seed)
    po = lone.astype(np.float64) - Ow[None, :]
    dist = np.linalg.norm(po, axis=1)
    at = np.sort(rng.choice(len(src), len(lone), replace=False))          # spread over the list
    pts["max_distance"], pts["min_distance"] = pts["max_distance"].copy(), pts["min_distance"].copy()
    for k, i in enumerate(at):
        pts["world_pos"][i] = lone[k]
        pts["normal"][i] = (po[k] / dist[k]).astype(np.float32)
        pts["max_distance"][i] = np.float32(dist[k] * 0.95)                # PredictScale: ceil(log(0.95) / log(sf)) = 0
        pts["min_distance"][i] = np.float32(dist[k] * 0.01)
        valid[i] = 1
    matched = np.where(rng.random(oF.c.N) < 0.2, HELD + np.arange(oF.c.N), -1).astype(np.int32)
    return pts, valid, Ow, matched


def random_case(name):
    """name -> dict(view(device) -> (oracle view, device view), points, valid, Tcw (ob.SE3), Ow, log_sf, matched, nleft, nlevels, expected)"""
    if name in _cases:
        return _cases[name]
    base = rc.random_case(name)
    pts, valid, Ow, matched = sim3_points(base, 21)
    oF, _ = base["view"](device=False)
    _cases[name] = dict(view=lambda device=True: base["view"](device=device), points=pts, valid=valid, Tcw=base["Tcw"], Ow=Ow,
                        log_sf=base["log_sf"], matched=matched, nleft=oF.c.N if oF.Nleft == -1 else oF.Nleft, nlevels=len(oF.sf), expected={})
    return _cases[name]


def expected(case, th, ratio, hand_pinhole, matched=None, tag=None, points=None, valid="case"):
    """the literal loop's result on a case (cached per parameter set; matched / points / valid other than the case's own under `tag`)"""
    key = (th, ratio, hand_pinhole, tag)
    if key not in case["expected"]:
        oF, _ = case["view"](device=False)
        case["expected"][key] = ref.search(oF, case["points"] if points is None else points, case["Tcw"], case["Ow"], case["log_sf"], th, ratio,
                                           case["matched"] if matched is None else matched, case["valid"] if isinstance(valid, str) else valid,
                                           hand_pinhole)
    return case["expected"][key]


def job_of(case, th, ratio, hand_pinhole, matched=None, points=None, valid="case"):
    """the orb.search_keyframe_sim3 job dict of a case"""
    from fasttrack_amd import orb
    return dict(points=case["points"] if points is None else points, Tcw=orb.SE3(case["Tcw"].q, case["Tcw"].t), Ow=case["Ow"],
                log_scale_factor=case["log_sf"], th=th, ratio_hamming=ratio, hand_pinhole=hand_pinhole,
                valid=case["valid"] if isinstance(valid, str) else valid, matched=case["matched"] if matched is None else matched)


def check_non_vacuous(name, case, r):
    """what a random case must exercise, on the literal loop's statistics"""
    st = r["stats"]
    M = len(case["valid"])
    assert st["changed_by_locks"] >= 50, (name, st)
    assert st["held_on_entry"] > 0, (name, st)
    assert all(st["stages"][s] > 0 for s in range(1, 8)), (name, st)
    assert len(st["levels"]) >= min(6, case["nlevels"]), (name, st)
    assert r["n_matches"] < st["walk"] < M, (name, r["n_matches"], st)


# ---- hand-built cases: fuse_cases' pinhole camera fx = fy = 400, cx, cy = 320, 240 on bounds (0, 0, 640, 480), identity pose, Ow = 0;
# a point made by hand_points(u, v, z, level) projects to (u, v) with PredictScale = level; cells are 10 x 10 pixels ----
BASE, flip, hand_keys, hand_points, hand_view, IDENTITY, LOG_SF = fc.BASE, fc.flip, fc.hand_keys, fc.hand_points, fc.hand_view, fc.IDENTITY, fc.LOG_SF


def hand_cases():
    """name -> dict(keys, desc, points, th, ratio, [matched, valid, keys_right, hand_pinhole],
    expect = dict(matched, point_keypoint, stage, n_matches)): the expectations are written out here from the reference text;
    test_sim3_search_cpu.py holds both restatements to them, the GPU test holds the library to the restatement AND to them"""
    c = {}
    pt = lambda u, v, d, z=5.0, level=0: (u, v, z, level, d)
    one = dict(keys=hand_keys([(300, 220)]), desc=[BASE[0]], th=3, ratio=1.0)
    c["match"] = dict(one, points=hand_points([pt(300, 220, flip(BASE[0], range(4)))]),
                      expect=dict(matched=[0], point_keypoint=[0], stage=[0], n_matches=1))
    # a point dropped by valid: isBad(), or already in vpMatched on entry
    c["not_valid"] = dict(one, points=hand_points([pt(300, 220, BASE[0])]), valid=[0],
                          expect=dict(matched=[-1], point_keypoint=[-1], stage=[1], n_matches=0))
    c["negative_depth"] = dict(one, points=hand_points([pt(300, 220, BASE[0], z=-5.0)]),
                               expect=dict(matched=[-1], point_keypoint=[-1], stage=[2], n_matches=0))
    edge = dict(keys=hand_keys([(639, 220), (1, 220)]), desc=[BASE[0], BASE[1]], th=3, ratio=1.0)
    c["u_equals_max_is_outside"] = dict(edge, points=hand_points([pt(640, 220, BASE[0])]),
                                        expect=dict(matched=[-1, -1], point_keypoint=[-1], stage=[3], n_matches=0))
    pd = hand_points([pt(300, 220, BASE[0])])
    pd["max_distance"] = (pd["max_distance"] * 0.1).astype(np.float32)
    c["beyond_max_distance"] = dict(one, points=pd, expect=dict(matched=[-1], point_keypoint=[-1], stage=[4], n_matches=0))
    axis = dict(keys=hand_keys([(320, 240)]), desc=[BASE[0]], th=3, ratio=1.0)
    c["dot_equals_half_dist_passes"] = dict(axis, points=hand_points([pt(320, 240, flip(BASE[0], range(7)), z=4.0)], normals=[[0, 0, 0.5]]),
                                            expect=dict(matched=[0], point_keypoint=[0], stage=[0], n_matches=1))
    c["dot_below_half_dist"] = dict(axis, points=hand_points([pt(320, 240, BASE[0], z=4.0)], normals=[[0, 0, 0.4999999]]),
                                    expect=dict(matched=[-1], point_keypoint=[-1], stage=[5], n_matches=0))
    # an empty window (6) against a window whose keypoints all lie outside the band (7: searched, nothing written)
    c["empty_window"] = dict(one, points=hand_points([pt(100, 100, BASE[0])]), expect=dict(matched=[-1], point_keypoint=[-1], stage=[6], n_matches=0))
    c["window_without_band"] = dict(keys=hand_keys([(300, 220)], octave=[3]), desc=[BASE[0]], th=3, ratio=1.0, points=hand_points([pt(300, 220, BASE[0])]),
                                    expect=dict(matched=[-1], point_keypoint=[-1], stage=[7], n_matches=0))
    # the band [level - 1, level] (:608): at level 0 octave 0 only (octave 1 holds the closest descriptor); at the last level 6 and 7
    c["level_zero_band"] = dict(keys=hand_keys([(300, 220), (301, 220)], octave=[1, 0]), desc=[BASE[0], flip(BASE[0], range(9))], th=3, ratio=1.0,
                                points=hand_points([pt(300.5, 220, BASE[0], level=0)]),
                                expect=dict(matched=[-1, 0], point_keypoint=[1], stage=[0], n_matches=1))
    c["last_level_band"] = dict(keys=hand_keys([(300, 220), (301, 220), (302, 220)], octave=[5, 6, 7]),
                                desc=[BASE[0], flip(BASE[0], range(5)), flip(BASE[0], range(9))], th=3, ratio=1.0,
                                points=hand_points([pt(301, 220, BASE[0], level=12)]),
                                expect=dict(matched=[-1, 0, -1], point_keypoint=[1], stage=[0], n_matches=1))
    # strict < (:615): of equal distances the first in GetFeaturesInArea's order - cell column, cell row, index
    tie = lambda xy, at: dict(keys=hand_keys(xy), desc=[flip(BASE[0], range(5)), flip(BASE[0], range(40, 45))], th=3, ratio=1.0,
                              points=hand_points([pt(at[0], at[1], BASE[0])]))
    c["tie_earlier_cell_column"] = dict(tie([(106, 100), (104, 100)], (105, 100)), expect=dict(matched=[-1, 0], point_keypoint=[1], stage=[0], n_matches=1))
    c["tie_earlier_cell_row"] = dict(tie([(100, 106), (100, 104)], (100, 105)), expect=dict(matched=[-1, 0], point_keypoint=[1], stage=[0], n_matches=1))
    c["tie_smaller_index"] = dict(tie([(101, 101), (100, 100)], (100.5, 100.5)), expect=dict(matched=[0, -1], point_keypoint=[0], stage=[0], n_matches=1))
    # two points with the same nearest keypoint: the second takes its next one (20 bits away, within 50) ...
    two = dict(keys=hand_keys([(300, 220), (302, 221)]), desc=[flip(BASE[0], range(3)), flip(BASE[0], range(30, 50))], th=3,
               points=hand_points([pt(301, 220.5, BASE[0]), pt(301, 220.5, BASE[0])]))
    c["second_point_takes_the_next"] = dict(two, ratio=1.0, expect=dict(matched=[0, 1], point_keypoint=[0, 1], stage=[0, 0], n_matches=2))
    # ... or nothing when that one is beyond the threshold (50 * 0.3f = 15)
    c["second_point_finds_none"] = dict(two, ratio=0.3, expect=dict(matched=[0, -1], point_keypoint=[0, -1], stage=[0, 7], n_matches=1))
    # a point above the threshold leaves its keypoint free for a later one
    c["above_threshold_leaves_free"] = dict(one, points=hand_points([pt(300, 220, flip(BASE[0], range(60))), pt(300, 220, flip(BASE[0], range(4)))]),
                                            expect=dict(matched=[1], point_keypoint=[-1, 0], stage=[7, 0], n_matches=1))
    # a keypoint held on entry is skipped whatever holds it (0 is a pointer too): the point takes the other one, or nothing
    held = dict(keys=hand_keys([(300, 220), (301, 220)]), desc=[BASE[0], flip(BASE[0], range(10))], th=3, ratio=1.0,
                points=hand_points([pt(300, 220, BASE[0])]))
    c["held_on_entry"] = dict(held, matched=[5, -1], expect=dict(matched=[5, 0], point_keypoint=[1], stage=[0], n_matches=1))
    c["held_by_point_zero"] = dict(held, matched=[0, 0], expect=dict(matched=[0, 0], point_keypoint=[-1], stage=[7], n_matches=0))
    # `bestDist<=TH_LOW*ratioHamming`: 50 * 1.5f = 75 counts, 76 does not; 50 * 1.0f = 50 counts, 51 does not
    for name, ratio, d in (("threshold_75_76", 1.5, 75), ("threshold_50_51", 1.0, 50)):
        c[name] = dict(keys=hand_keys([(100, 100), (300, 300)]), desc=[flip(BASE[0], range(d)), flip(BASE[1], range(d + 1))], th=3, ratio=ratio,
                       points=hand_points([pt(100, 100, BASE[0]), pt(300, 300, BASE[1])]),
                       expect=dict(matched=[0, -1], point_keypoint=[0, -1], stage=[0, 7], n_matches=1))
    # a two-camera keyframe: GetFeaturesInArea looks at the left camera only; the right keypoint at the second point's place (with the
    # point's own descriptor) is never seen, and the entries >= NLeft stay as they were
    c["two_cameras"] = dict(keys=hand_keys([(300, 220), (10, 10)]), keys_right=hand_keys([(50, 50), (300, 220)]),
                            desc=[BASE[0], BASE[1], BASE[2], flip(BASE[0], range(6))], th=3, ratio=1.0, matched=[-1, -1, 9, -1],
                            points=hand_points([pt(300, 220, flip(BASE[0], range(6))), pt(50, 50, BASE[2])]),
                            expect=dict(matched=[0, -1, 9, -1], point_keypoint=[0, -1], stage=[0, 6], n_matches=1))
    # six keypoints of one cell, 0 .. 5 bits from the descriptor all six points carry: point j takes keypoint j; the fifth and sixth
    # find their four nearest taken (the library's top record holds four)
    six = [(300.2 + 0.03 * k, 220.2) for k in range(6)]
    c["past_the_top_record"] = dict(keys=hand_keys(six), desc=[flip(BASE[0], range(k)) for k in range(6)], th=3, ratio=1.0,
                                    points=hand_points([pt(300.3, 220.2, BASE[0])] * 6),
                                    expect=dict(matched=list(range(6)), point_keypoint=list(range(6)), stage=[0] * 6, n_matches=6))
    for v in c.values():
        v.setdefault("matched", [-1] * (len(v["keys"]) + (0 if v.get("keys_right") is None else len(v["keys_right"]))))
        v.setdefault("valid", None)
        v.setdefault("keys_right", None)
        v.setdefault("hand_pinhole", False)
    return c


def crowd_case(n):
    """One grid cell (10 x 10 pixels at (300, 220)) with n keypoints of octave 0, 0.03 px apart inside the 3-pixel box of n points that
    all aim at the cell with one descriptor, the keypoints' 1 .. 40 bits from it (the nearest in the middle of the list, ties broken
    by the index): every point writes, and from the fifth on its four nearest keypoints are taken -> a hand case without expectation"""
    xy = [(300.2 + 0.03 * (k % 17), 220.2 + 0.03 * (k // 17)) for k in range(n)]
    desc = [flip(BASE[0], range(1 + (abs(k - n // 2) // 2) % 40)) for k in range(n)]
    return dict(keys=hand_keys(xy), desc=desc, th=3, ratio=1.0, points=hand_points([(300.4, 220.4, 5.0, 0, BASE[0])] * n), matched=[-1] * n,
                valid=None, keys_right=None, hand_pinhole=False)


def hand_job(case, hand_pinhole=None):
    from fasttrack_amd import orb
    return dict(points=case["points"], Tcw=orb.SE3(IDENTITY.q, IDENTITY.t), Ow=np.zeros(3, np.float32), log_scale_factor=LOG_SF, th=case["th"],
                ratio_hamming=case["ratio"], hand_pinhole=case["hand_pinhole"] if hand_pinhole is None else hand_pinhole, valid=case["valid"],
                matched=np.array(case["matched"], np.int32))


def run_hand_case(case, fn=ref.search, hand_pinhole=None):
    oF, _ = hand_view(case["keys"], case["desc"], keys_right=case["keys_right"])
    return fn(oF, case["points"], IDENTITY, np.zeros(3, np.float32), LOG_SF, case["th"], case["ratio"], np.array(case["matched"], np.int32),
              case["valid"], case["hand_pinhole"] if hand_pinhole is None else hand_pinhole)


def overload_case():
    """A point whose u differs by an ulp between mpCamera->project and the projection written out (found by a seeded search), and a
    keypoint exactly 3 pixels (the radius at level 0) right of the smaller u: outside the box `fabs(dx) < r` of the form that gives the
    smaller u, inside the other's.  -> (hand case without expectation, the form that sees the keypoint)"""
    rng = np.random.default_rng(77)
    f32 = np.float32
    for _ in range(100000):
        u, v = rng.uniform(260, 500), rng.uniform(100, 400)         # (u + 3 stays in the binade [256, 512): the sums below are exact)
        P = hand_points([(u, v, 5.0, 0, BASE[0])])
        X, Y, Z = [f32(c) for c in P["world_pos"][0]]
        ua, va = f32(f32(f32(400.0) * X) / Z + f32(320.0)), f32(f32(f32(400.0) * Y) / Z + f32(240.0))
        invz = f32(f32(1.0) / Z)
        ub, vb = f32(f32(400.0) * f32(X * invz) + f32(320.0)), f32(f32(400.0) * f32(Y * invz) + f32(240.0))
        if ua != ub and abs(float(ua) - float(ub)) < 1e-3:
            lo = min(ua, ub)
            kx = f32(lo + f32(3.0))
            assert float(kx) - float(lo) == 3.0
            case = dict(keys=hand_keys([(float(kx), float(va))]), desc=[flip(BASE[0], range(2))], th=3, ratio=1.0, points=P, matched=[-1],
                        valid=None, keys_right=None, hand_pinhole=False)
            return case, bool(ub > ua)
    raise AssertionError("no point tells the projections apart")

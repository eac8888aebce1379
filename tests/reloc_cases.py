"""Inputs of the SearchByProjection(Frame, KeyFrame) tests (test_reloc_search_cpu.py, test_gpu_reloc_search.py): seeded random
cases on the frames of tests/scenarios.py and hand-built cases of a dozen keypoints, each with the restatement's result
(tests/reloc_search_ref.py) computed once and shared.

A random case: the keyframe's points are last_frame_scenario's world points of the frame's own keypoints, taken twice - every
keypoint once, then as many random repeats moved by 1 cm of noise, so that windows collide and later points find their nearest
keypoint taken; max_distance = |X| * sf[octave] * U(0.7, 1.5), min_distance = max_distance / sf[nlevels - 1]; 85 % of the points
valid; 20 % of the keypoints held on entry with Observations() in {0, 1, 2}; the pose a random_se3 step.
"""
import numpy as np

from oracle import binding as ob
from tests import reloc_search_ref as ref
from tests import scenarios as sc

KP = ob.KP_DTYPE
KB8_CAM_256 = [95.489, 95.4865, 127.465, 128.45, 0.0034, 0.0007, -0.0020, 0.00020]   # sc.KB8_CAM for a 256 x 256 image


def kb8_unproject(cam, u, v):
    """unit-z rays of KannalaBrandt8 pixels (float64, Newton on r(theta)); theta stays below pi / 2 for the frames used here"""
    mx, my = (np.asarray(u, np.float64) - cam[2]) / cam[0], (np.asarray(v, np.float64) - cam[3]) / cam[1]
    r = np.sqrt(mx * mx + my * my)
    th = r.copy()
    for _ in range(20):
        t2 = th * th
        f = th * (1 + t2 * (cam[4] + t2 * (cam[5] + t2 * (cam[6] + t2 * cam[7])))) - r
        df = 1 + t2 * (3 * cam[4] + t2 * (5 * cam[5] + t2 * (7 * cam[6] + t2 * 9 * cam[7])))
        th = th - f / df
    s = np.where(r > 1e-12, np.tan(th) / np.maximum(r, 1e-12), 1.0)
    return mx * s, my * s


def keyframe_points(keys, desc, sf, intr, w, h, seed, kb8_cam=None):
    """-> (kf dict, Tcw as (q, t)) as the module docstring says"""
    N, nlevels = len(keys), len(sf)
    last, _ = sc.last_frame_scenario(keys, desc, None, np.zeros(N, np.float32), intr, w, h, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    world = last["world_pos"].astype(np.float32)
    if kb8_cam is not None:
        rx, ry = kb8_unproject(kb8_cam, keys["x"], keys["y"])
        z = world[:, 2].astype(np.float64)
        world = np.stack([rx * z, ry * z, z], 1).astype(np.float32)
    rep = rng.integers(0, N, N)
    src = np.concatenate([np.arange(N), rep])
    world = np.concatenate([world, world[rep] + rng.normal(0, 0.01, (N, 3))]).astype(np.float32)
    M = len(src)
    max_d = (np.linalg.norm(world, axis=1) * sf[keys["octave"][src]] * rng.uniform(0.7, 1.5, M)).astype(np.float32)
    kf = dict(valid=(rng.random(M) < 0.85).astype(np.uint8), world_pos=world, max_distance=max_d,
              min_distance=(max_d / sf[nlevels - 1]).astype(np.float32), descriptors=last["descriptors"][src].copy(),
              observations=last["observations"][src].astype(np.int32), angle=last["angle"][src].astype(np.float32))
    return kf, sc.random_se3(rng)


def holder_on_entry(n, seed):
    rng = np.random.default_rng(seed + 2000)
    return np.where(rng.random(n) < 0.2, rng.integers(0, 3, n), -1).astype(np.int32)


_cases = {}


def random_case(name):
    """name -> dict(fr, bounds, kf, Tcw (ob.SE3), holder, log_sf, view(uright=..., device=...) -> (oracle view, device view))"""
    if name in _cases:
        return _cases[name]
    kind = name.split(":")
    if kind[0] == "pinhole":                       # pinhole:<w>x<h>:<nf>:<seed>
        w, h = [int(v) for v in kind[1].split("x")]
        nf, seed = int(kind[2]), int(kind[3])
        fr = sc.geometry_frame(w, h, nf, seed)
        bounds = sc.frame_bounds(w, h)
        kf, (q, t) = keyframe_points(fr["kL"], fr["dL"], fr["sf"], fr["intr"], w, h, seed)
        holder = holder_on_entry(len(fr["kL"]), seed)
        view = lambda uright=True, device=True: sc.geometry_views(fr, bounds, uright=uright, holder=holder, device=device)
    elif kind[0] == "geometry":                    # geometry:<bounds>:<scale factor>:<levels>: the frames of sc.geometry_case
        gc = sc.geometry_case(kind[1], float(kind[2]), int(kind[3]))
        fr, bounds = gc["fr"], gc["bounds"]
        kf, (q, t) = keyframe_points(fr["kL"], fr["dL"], fr["sf"], fr["intr"], fr["w"], fr["h"], 17)
        holder = holder_on_entry(len(fr["kL"]), 17)
        view = lambda uright=True, device=True: sc.geometry_views(fr, bounds, uright=uright, holder=holder, device=device)
    elif kind[0] == "kb8mono":                     # a KannalaBrandt8 frame with one camera, 256 x 256
        fr = sc.geometry_frame(256, 256, 600, 9)
        bounds = sc.frame_bounds(256, 256)
        intr = dict(fx=KB8_CAM_256[0], fy=KB8_CAM_256[1], cx=KB8_CAM_256[2], cy=KB8_CAM_256[3])
        kf, (q, t) = keyframe_points(fr["kL"], fr["dL"], fr["sf"], intr, 256, 256, 9, kb8_cam=KB8_CAM_256)
        holder = holder_on_entry(len(fr["kL"]), 9)

        def view(uright=False, device=True):
            kw = dict(keys=fr["kL"], descriptors=fr["dL"], bounds=bounds, cam_model=1, cam=KB8_CAM_256, holder_obs=holder)
            gF = None
            if device:
                from fasttrack_amd import orb
                gF = orb.FrameView(scale_factors=fr["sf"], **kw)
            return ob.FrameView(scale_factors_=fr["sf"], **kw), gF
    elif kind[0] == "kb8two":                      # the two-camera KannalaBrandt8 frame, 512 x 512
        fr = sc.geometry_frame(512, 512, 1000, 12, two_cameras=True)
        bounds = sc.frame_bounds(512, 512)
        kf, (q, t) = keyframe_points(fr["kL"], fr["dL"], fr["sf"], fr["kb8_intr"], 512, 512, 12, kb8_cam=sc.KB8_CAM)
        holder = holder_on_entry(len(fr["kL"]) + len(fr["kR"]), 12)
        view = lambda uright=True, device=True: sc.geometry_views(fr, bounds, holder=holder, device=device)
    else:
        raise KeyError(name)
    _cases[name] = dict(fr=fr, bounds=bounds, kf=kf, Tcw=ob.SE3(q, t), holder=holder, log_sf=fr["log_sf"], view=view, expected={})
    return _cases[name]


def expected(case, th, orb_dist, check_orientation=True, kf=None, holder=None, tag=None):
    """the restatement's result on a case (cached per parameter set; kf / holder: other than the case's own, under `tag`)"""
    key = (th, orb_dist, check_orientation, tag)
    if key not in case["expected"]:
        oF, _ = case["view"](device=False)
        if holder is not None:
            oF.holder_obs[:] = holder
        case["expected"][key] = ref.search_by_projection(oF, case["kf"] if kf is None else kf, case["Tcw"], case["log_sf"], th, orb_dist,
                                                         check_orientation)
    return case["expected"][key]


# ---- hand-built cases: a pinhole camera fx = fy = 400, cx, cy = 320, 240 on bounds (0, 0, 640, 480), the identity pose ----
W, H = 640, 480
CAM = [400.0, 400.0, 320.0, 240.0]
SF, _ = ob.scale_factors(1.2, 8)
LOG_SF = float(np.float32(np.log(np.float32(1.2))))
IDENTITY = (np.array([0, 0, 0, 1], np.float32), np.zeros(3, np.float32))
BASE = np.random.default_rng(7).integers(0, 256, (64, 32), dtype=np.uint8)   # pairwise about 128 bits apart


def flip(d, bits):
    d = d.copy()
    for b in bits:
        d[b // 8] ^= 1 << (b % 8)
    return d


def hand_keys(xy, octave=None, angle=None):
    k = np.zeros(len(xy), KP)
    k["x"], k["y"] = [p[0] for p in xy], [p[1] for p in xy]
    k["size"] = 31
    k["octave"] = 0 if octave is None else octave
    k["angle"] = 0 if angle is None else angle
    return k


def hand_points(spec):
    """spec: (u, v, z, level, descriptor, observations, angle) per point: the point that projects to (u, v) from depth z (z < 0:
    behind the camera) under the identity pose, with max_distance = |X| * 1.2 ^ (level - 0.5), so that PredictScale gives `level`"""
    n = len(spec)
    world = np.array([[(s[0] - CAM[2]) / CAM[0] * s[2], (s[1] - CAM[3]) / CAM[1] * s[2], s[2]] for s in spec], np.float32).reshape(n, 3)
    dist = np.linalg.norm(world.astype(np.float64), axis=1)
    max_d = np.array([d * 1.2 ** (s[3] - 0.5) for d, s in zip(dist, spec)], np.float32)
    return dict(valid=np.ones(n, np.uint8), world_pos=world, max_distance=max_d, min_distance=(max_d * 1e-3).astype(np.float32),
                descriptors=np.stack([s[4] for s in spec]).astype(np.uint8), observations=np.array([s[5] for s in spec], np.int32),
                angle=np.array([s[6] for s in spec], np.float32))


def hand_view(keys, desc, holder=None, uright=None, device=False):
    kw = dict(keys=keys, descriptors=np.asarray(desc, np.uint8).reshape(len(keys), 32), bounds=(0, 0, W, H), cam=CAM, holder_obs=holder,
              uright=uright)
    gF = None
    if device:
        from fasttrack_amd import orb
        gF = orb.FrameView(scale_factors=SF, **kw)
    return ob.FrameView(scale_factors_=SF, **kw), gF


def hand_cases():
    """name -> dict(keys, desc, holder, kf, th, orb_dist, check_orientation, expect=dict(assign, n, best_dist, best_idx, holder_obs)):
    the expectations are written out here from the reference text; test_reloc_search_cpu.py holds the restatement to them, the GPU
    test holds the library to the restatement AND to them"""
    c = {}
    pt = lambda u, v, d, z=5.0, level=0, obs=3, angle=0.0: (u, v, z, level, d, obs, angle)
    # a holder with 0 observations locks its keypoint (:2150 tests the pointer, not Observations())
    c["zero_obs_holder_locks"] = dict(keys=hand_keys([(300, 220)]), desc=[BASE[0]], holder=[0], kf=hand_points([pt(300, 220, BASE[0])]),
                                      th=10, orb_dist=100, expect=dict(assign=[-1], n=0, best_dist=[256], best_idx=[-1], holder_obs=[0]))
    c["free_keypoint_is_taken"] = dict(keys=hand_keys([(300, 220)]), desc=[BASE[0]], holder=[-1], kf=hand_points([pt(300, 220, BASE[0])]),
                                       th=10, orb_dist=100, expect=dict(assign=[0], n=1, best_dist=[0], best_idx=[0], holder_obs=[3]))
    # no depth test (:2112-2119): a point behind the camera whose pinhole projection lands inside the bounds is searched
    c["behind_the_camera"] = dict(keys=hand_keys([(300, 220)]), desc=[BASE[0]], holder=[-1], kf=hand_points([pt(300, 220, flip(BASE[0], range(4)), z=-5.0)]),
                                  th=10, orb_dist=100, expect=dict(assign=[0], n=1, best_dist=[4], best_idx=[0], holder_obs=[3]))
    # strict < (:2157): of equal distances the first in GetFeaturesInArea's order wins - keypoint 1 in the earlier cell column
    c["tie_earlier_cell_column"] = dict(keys=hand_keys([(120, 100), (100, 100)]), desc=[flip(BASE[0], range(5)), flip(BASE[0], range(40, 45))],
                                        holder=[-1, -1], kf=hand_points([pt(110, 100, BASE[0])]), th=15, orb_dist=100,
                                        expect=dict(assign=[-1, 0], n=1, best_dist=[5], best_idx=[1], holder_obs=[-1, 3]))
    # the same cell column, the earlier cell row; and the same cell, the smaller index
    c["tie_earlier_cell_row"] = dict(keys=hand_keys([(100, 120), (100, 100)]), desc=[flip(BASE[0], range(5)), flip(BASE[0], range(40, 45))],
                                     holder=[-1, -1], kf=hand_points([pt(100, 110, BASE[0])]), th=15, orb_dist=100,
                                     expect=dict(assign=[-1, 0], n=1, best_dist=[5], best_idx=[1], holder_obs=[-1, 3]))
    c["tie_smaller_index"] = dict(keys=hand_keys([(101, 101), (100, 100)]), desc=[flip(BASE[0], range(5)), flip(BASE[0], range(40, 45))],
                                  holder=[-1, -1], kf=hand_points([pt(100, 100, BASE[0])]), th=15, orb_dist=100,
                                  expect=dict(assign=[0, -1], n=1, best_dist=[5], best_idx=[0], holder_obs=[3, -1]))
    # two points with the same nearest keypoint: the second takes its next one ...
    two = dict(keys=hand_keys([(300, 220), (304, 222)]), desc=[flip(BASE[0], range(3)), flip(BASE[0], range(30, 50))], holder=[-1, -1],
               kf=hand_points([pt(301, 221, BASE[0], obs=1), pt(301, 221, BASE[0], obs=2)]), th=10)
    c["second_point_takes_the_next"] = dict(two, orb_dist=100, expect=dict(assign=[0, 1], n=2, best_dist=[3, 20], best_idx=[0, 1], holder_obs=[1, 2]))
    # ... or none when that one is beyond ORBdist (the loop still leaves bestDist / bestIdx2 of the free candidate)
    c["second_point_finds_none"] = dict(two, orb_dist=10, expect=dict(assign=[0, -1], n=1, best_dist=[3, 20], best_idx=[0, 1], holder_obs=[1, -1]))
    # bestDist <= ORBdist (:2164)
    c["orb_dist_inclusive"] = dict(keys=hand_keys([(100, 100), (300, 300)]), desc=[flip(BASE[0], range(64)), flip(BASE[1], range(65))],
                                   holder=[-1, -1], kf=hand_points([pt(100, 100, BASE[0]), pt(300, 300, BASE[1])]), th=3, orb_dist=64,
                                   expect=dict(assign=[0, -1], n=1, best_dist=[64, 65], best_idx=[0, 1], holder_obs=[3, -1]))
    # level 0 searches octaves 0 - 1 (nPredictedLevel - 1 = -1), the last level octaves nlevels - 2 .. nlevels - 1: the closest
    # descriptor sits on the octave just outside the band
    c["level_zero_band"] = dict(keys=hand_keys([(300, 220), (301, 220), (302, 220)], octave=[2, 1, 0]),
                                desc=[BASE[0], flip(BASE[0], range(5)), flip(BASE[0], range(9))], holder=[-1, -1, -1],
                                kf=hand_points([pt(301, 220, BASE[0], level=0)]), th=10, orb_dist=100,
                                expect=dict(assign=[-1, 0, -1], n=1, best_dist=[5], best_idx=[1], holder_obs=[-1, 3, -1]))
    c["last_level_band"] = dict(keys=hand_keys([(300, 220), (301, 220), (302, 220)], octave=[5, 6, 7]),
                                desc=[BASE[0], flip(BASE[0], range(5)), flip(BASE[0], range(9))], holder=[-1, -1, -1],
                                kf=hand_points([pt(301, 220, BASE[0], level=12)]), th=10, orb_dist=100,
                                expect=dict(assign=[-1, 0, -1], n=1, best_dist=[5], best_idx=[1], holder_obs=[-1, 3, -1]))
    # An entry the histogram removes had locked its keypoint during the loop: point 0 (150 degrees: a bin of its own, 1 < 0.1f * 12)
    # takes keypoint 0, points 1 .. 12 (bin 0) take keypoints 1 .. 12, point 13 (bin 0) finds keypoint 0 - its only candidate - held.
    # After the removal keypoint 0 is free again (assign, holder_obs), and point 13 stays unmatched.
    nk = 13
    keys = hand_keys([(40 + 40 * t, 100) for t in range(nk)])
    spec = [pt(40, 100, BASE[0], angle=150.0)] + [pt(40 + 40 * t, 100, BASE[t], angle=0.0) for t in range(1, nk)] + \
           [pt(40, 100, flip(BASE[0], range(2)), angle=0.0)]
    c["histogram_removal_had_locked"] = dict(keys=keys, desc=BASE[:nk], holder=[-1] * nk, kf=hand_points(spec), th=10, orb_dist=100,
                                             expect=dict(assign=[-1] + list(range(1, nk)), n=12, best_dist=[0] * nk + [256],
                                                         best_idx=list(range(nk)) + [-1], holder_obs=[-1] + [3] * 12))
    for v in c.values():
        v.setdefault("check_orientation", True)
    return c


def run_hand_case(case):
    oF, _ = hand_view(case["keys"], case["desc"], np.array(case["holder"], np.int32))
    return ref.search_by_projection(oF, case["kf"], ob.SE3(*IDENTITY), LOG_SF, case["th"], case["orb_dist"], case["check_orientation"])


def capacity_case(n_cell=300, n_points=5):
    """One grid cell with n_cell keypoints of one descriptor (10 x 10 pixels, positions 0.03 px apart) and n_points points aimed
    at it: more candidates per point than a segment of 256 holds"""
    xy = [(300.0 + 0.03 * (k % 17), 220.0 + 0.03 * (k // 17)) for k in range(n_cell)]
    pt = lambda d: (300.2, 220.2, 5.0, 0, d, 2, 0.0)
    return dict(keys=hand_keys(xy), desc=np.repeat(BASE[:1], n_cell, axis=0), holder=[-1] * n_cell,
                kf=hand_points([pt(flip(BASE[0], range(k))) for k in range(n_points)]), th=10, orb_dist=100, check_orientation=True)

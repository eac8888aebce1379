"""Inputs of the ORBmatcher::Fuse tests (test_fuse_cpu.py, test_gpu_fuse.py): seeded random cases on the frames of
reloc_cases.random_case (its geometry:<bounds>:<scale factor>:<levels> frames included) and hand-built cases of a few keypoints, each with the restatement's result (tests/fuse_ref.py) computed
once and shared.

A random case: the points are reloc_cases.keyframe_points of the searched camera's keypoints (every keypoint once, then as many
repeats moved by 1 cm) with normals unit(PO) + N(0, 0.6) per coordinate, normalised again; 5 % of the points are reflected through
the camera centre (behind the camera), 5 % moved sideways by 4 |z| + 1 (outside the image); `valid` is the points' own (85 %).
"""
import numpy as np

from oracle import binding as ob
from tests import fuse_ref as ref
from tests import reloc_cases as rc
from tests import reloc_search_ref as rref
from tests import scenarios as sc

RANDOM = ["pinhole:320x240:500:5", "kb8mono", "kb8two", "kb8two:right"]
_cases = {}


def fuse_points(kf, Tcw, seed):
    """reloc_cases' keyframe points as Fuse's: normals, the reflected and the shifted twentieths -> (points dict, valid, Ow)"""
    rng = np.random.default_rng(seed + 3000)
    Ow = rref.camera_centre(Tcw)
    world = kf["world_pos"].astype(np.float32).copy()
    M = len(world)
    pick = rng.random(M)
    behind, aside = pick < 0.05, (pick >= 0.05) & (pick < 0.10)
    world[behind] = (2 * Ow[None, :] - world[behind]).astype(np.float32)
    world[aside, 0] += (4 * np.abs(world[aside, 2]) + 1).astype(np.float32)
    po = world.astype(np.float64) - Ow[None, :]
    n = po / np.linalg.norm(po, axis=1)[:, None] + rng.normal(0, 0.6, (M, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    pts = dict(world_pos=world, normal=n.astype(np.float32), max_distance=kf["max_distance"], min_distance=kf["min_distance"],
               descriptors=kf["descriptors"])
    return pts, kf["valid"].copy(), Ow


def random_case(name):
    """name -> dict(view(device) -> (oracle view, device view), points, valid, Tcw (ob.SE3), Ow, log_sf, right, cam2, expected)"""
    if name in _cases:
        return _cases[name]
    right = name.endswith(":right")
    base = rc.random_case(name.split(":right")[0])
    fr = base["fr"]
    if right:   # the right camera's own keypoints seen from the pose as the right camera's (any SE3 serves)
        kf, (q, t) = rc.keyframe_points(fr["kR"], fr["dR"], fr["sf"], fr["kb8_intr"], 512, 512, 13, kb8_cam=sc.KB8_CAM)
        Tcw, seed = ob.SE3(q, t), 13
    else:
        kf, Tcw, seed = base["kf"], base["Tcw"], 12
    pts, valid, Ow = fuse_points(kf, Tcw, seed)
    _cases[name] = dict(view=lambda device=True: base["view"](device=device), points=pts, valid=valid, Tcw=Tcw, Ow=Ow, log_sf=base["log_sf"],
                        right=right, cam2=list(sc.KB8_CAM) if right else None, expected={})
    return _cases[name]


def expected(case, th, check_reprojection):
    key = (th, check_reprojection)
    if key not in case["expected"]:
        oF, _ = case["view"](device=False)
        case["expected"][key] = ref.fuse(oF, case["points"], case["Tcw"], case["Ow"], case["log_sf"], th, case["right"], case["cam2"],
                                         case["valid"], check_reprojection)
    return case["expected"][key]


def target_of(case, gF, th, check_reprojection, valid="case"):
    """the orb.fuse_search target dict of a case on the device view gF"""
    from fasttrack_amd import orb
    return dict(kf=gF, Tcw=orb.SE3(case["Tcw"].q, case["Tcw"].t), Ow=case["Ow"], log_scale_factor=case["log_sf"], th=th,
                right=case["right"], cam2=case["cam2"], valid=case["valid"] if isinstance(valid, str) else valid,
                check_reprojection=check_reprojection)


# ---- hand-built cases: reloc_cases' pinhole camera fx = fy = 400, cx, cy = 320, 240 on bounds (0, 0, 640, 480), identity pose, so
# that Ow = 0, PO = the point and a point made by hand_points(u, v, z, level) projects to (u, v) with PredictScale = level ----
W, H, CAM, SF, LOG_SF, BASE, flip, hand_keys = rc.W, rc.H, rc.CAM, rc.SF, rc.LOG_SF, rc.BASE, rc.flip, rc.hand_keys
IDENTITY = ob.SE3(*rc.IDENTITY)
MBF = 40.0


def hand_points(spec, normals=None):
    """spec: (u, v, z, level, descriptor) per point -> Fuse's points; the normal is unit(PO) unless given"""
    kf = rc.hand_points([(s[0], s[1], s[2], s[3], s[4], 1, 0.0) for s in spec])
    w = kf["world_pos"].astype(np.float64)
    n = w / np.maximum(np.linalg.norm(w, axis=1), 1e-30)[:, None] if normals is None else np.asarray(normals, np.float64)
    return dict(world_pos=kf["world_pos"], normal=n.astype(np.float32), max_distance=kf["max_distance"], min_distance=kf["min_distance"],
                descriptors=kf["descriptors"])


def hand_view(keys, desc, uright=None, device=False, keys_right=None, sf=None):
    sf = SF if sf is None else sf
    n = len(keys) + (0 if keys_right is None else len(keys_right))
    kw = dict(keys=keys, descriptors=np.asarray(desc, np.uint8).reshape(n, 32), bounds=(0, 0, W, H), cam=CAM, uright=uright, mbf=MBF)
    if keys_right is not None:
        kw.update(keys_right=keys_right, left_to_right=np.full(len(keys), -1, np.int32), right_to_left=np.full(len(keys_right), -1, np.int32))
    gF = None
    if device:
        from fasttrack_amd import orb
        gF = orb.FrameView(scale_factors=sf, **kw)
    return ob.FrameView(scale_factors_=sf, **kw), gF


def hand_cases():
    """name -> dict(keys, desc, points, th, [uright, keys_right, right, check_reprojection, valid],
    expect = dict(best_idx, best_dist, stage, n_found)): the expectations are written out here from the reference text;
    test_fuse_cpu.py holds the restatement to them, the GPU test holds the library to the restatement AND to them"""
    c = {}
    pt = lambda u, v, d, z=5.0, level=0: (u, v, z, level, d)
    one = dict(keys=hand_keys([(300, 220)]), desc=[BASE[0]], th=3)
    c["match"] = dict(one, points=hand_points([pt(300, 220, flip(BASE[0], range(4)))]), expect=dict(best_idx=[0], best_dist=[4], stage=[0], n_found=1))
    c["not_valid"] = dict(one, points=hand_points([pt(300, 220, BASE[0])]), valid=[0], expect=dict(best_idx=[-1], best_dist=[256], stage=[1], n_found=0))
    c["negative_depth"] = dict(one, points=hand_points([pt(300, 220, BASE[0], z=-5.0)]), expect=dict(best_idx=[-1], best_dist=[256], stage=[2], n_found=0))
    # z exactly 0 passes `p3Dc(2)<0.0f`; invz = inf, the pinhole projection is inf or NaN and IsInImage fails (:1312)
    p0 = hand_points([pt(300, 220, BASE[0])])
    p0["world_pos"] = np.array([[1.0, 1.0, 0.0]], np.float32)
    c["depth_zero"] = dict(one, points=p0, expect=dict(best_idx=[-1], best_dist=[256], stage=[3], n_found=0))
    p00 = hand_points([pt(300, 220, BASE[0])])
    p00["world_pos"] = np.array([[0.0, 0.0, -0.0]], np.float32)   # 0 / -0 = NaN: fails IsInImage as well
    c["depth_minus_zero"] = dict(one, points=p00, expect=dict(best_idx=[-1], best_dist=[256], stage=[3], n_found=0))
    # IsInImage: u == mnMaxX is outside, u == mnMinX inside (x = (u - 320) / 400 * 5 = +-4 is exact at z = 5, and 400 * 4 / 5 + 320 = 640)
    edge = dict(keys=hand_keys([(639, 220), (1, 220)]), desc=[BASE[0], BASE[1]], th=3)
    c["u_equals_max_is_outside"] = dict(edge, points=hand_points([pt(640, 220, BASE[0])]),
                                        expect=dict(best_idx=[-1], best_dist=[256], stage=[3], n_found=0))
    c["u_equals_min_is_inside"] = dict(edge, points=hand_points([pt(0, 220, flip(BASE[1], range(2)))]),
                                       expect=dict(best_idx=[1], best_dist=[2], stage=[0], n_found=1))
    # the distance range: max_distance = |X| * 1.2 ^ (level - 0.5); a tenth of it is below dist3D / 1.2
    pd = hand_points([pt(300, 220, BASE[0])])
    pd["max_distance"] = (pd["max_distance"] * 0.1).astype(np.float32)
    c["beyond_max_distance"] = dict(one, points=pd, expect=dict(best_idx=[-1], best_dist=[256], stage=[4], n_found=0))
    # PO.dot(Pn) < 0.5 * dist3D: PO = (0, 0, 4), dist3D = 4; Pn = (0, 0, 0.5) gives dot = 2 = 0.5 * 4 exactly: not less, passes
    axis = dict(keys=hand_keys([(320, 240)]), desc=[BASE[0]], th=3)
    c["dot_equals_half_dist_passes"] = dict(axis, points=hand_points([pt(320, 240, flip(BASE[0], range(7)), z=4.0)], normals=[[0, 0, 0.5]]),
                                            expect=dict(best_idx=[0], best_dist=[7], stage=[0], n_found=1))
    c["dot_below_half_dist"] = dict(axis, points=hand_points([pt(320, 240, BASE[0], z=4.0)], normals=[[0, 0, 0.4999999]]),
                                    expect=dict(best_idx=[-1], best_dist=[256], stage=[5], n_found=0))
    # an empty window (6) against a window whose keypoints all lie outside the band (0, nothing found)
    c["empty_window"] = dict(one, points=hand_points([pt(100, 100, BASE[0])]), expect=dict(best_idx=[-1], best_dist=[256], stage=[6], n_found=0))
    c["window_without_band"] = dict(keys=hand_keys([(300, 220)], octave=[3]), desc=[BASE[0]], th=3, points=hand_points([pt(300, 220, BASE[0])]),
                                    expect=dict(best_idx=[-1], best_dist=[256], stage=[0], n_found=0))
    # the band [level - 1, level]: at level 0 octave 0 only (octave 1 holds the closest descriptor), at the last level (7) octaves 6
    # and 7 (octave 5 holds the closest); radius = 3 * sf[level]
    c["level_zero_band"] = dict(keys=hand_keys([(300, 220), (301, 220)], octave=[1, 0]), desc=[BASE[0], flip(BASE[0], range(9))], th=3,
                                points=hand_points([pt(300.5, 220, BASE[0], level=0)]), expect=dict(best_idx=[1], best_dist=[9], stage=[0], n_found=1))
    c["last_level_band"] = dict(keys=hand_keys([(300, 220), (301, 220), (302, 220)], octave=[5, 6, 7]),
                                desc=[BASE[0], flip(BASE[0], range(5)), flip(BASE[0], range(9))], th=3,
                                points=hand_points([pt(301, 220, BASE[0], level=12)]), expect=dict(best_idx=[1], best_dist=[5], stage=[0], n_found=1))
    # The chi-square test.  Point at (300, 220), z = 5, level 0 (inverse sigma 1): ur = 300 - 40 / 5 = 292.  Keypoint 0 at (302, 221):
    # ex = -2, ey = -1, e2 = 5 <= 5.99 as a mono keypoint; with uright = 290.5, er = 1.5, e2 = 7.25 <= 7.8: passes; with uright = 290,
    # er = 2, e2 = 9 > 7.8: rejected, and keypoint 1 at (301, 220) (e2 = 1 + 1 with uright 291) takes the point with a farther descriptor.
    chi = dict(keys=hand_keys([(302, 221), (301, 220)]), desc=[flip(BASE[0], range(2)), flip(BASE[0], range(30))], th=3,
               points=hand_points([pt(300, 220, BASE[0])]))
    c["chi2_stereo_rejects_the_closest"] = dict(chi, uright=[290.0, 291.0], expect=dict(best_idx=[1], best_dist=[30], stage=[0], n_found=1))
    c["chi2_stereo_passes"] = dict(chi, uright=[290.5, 291.0], expect=dict(best_idx=[0], best_dist=[2], stage=[0], n_found=1))
    c["chi2_same_geometry_passes_mono"] = dict(chi, uright=[-1.0, -1.0], expect=dict(best_idx=[0], best_dist=[2], stage=[0], n_found=1))
    # a mono keypoint at (302.5, 221): e2 = 6.25 + 1 > 5.99 rejected, although inside the 3-pixel box
    c["chi2_mono_rejects"] = dict(keys=hand_keys([(302.5, 221), (301, 220)]), desc=[flip(BASE[0], range(2)), flip(BASE[0], range(30))], th=3,
                                  points=hand_points([pt(300, 220, BASE[0])]), expect=dict(best_idx=[1], best_dist=[30], stage=[0], n_found=1))
    # the Sim3 overload knows neither the chi-square test nor mvuRight
    c["sim3_ignores_chi2_and_uright"] = dict(chi, uright=[290.0, 291.0], check_reprojection=False,
                                             expect=dict(best_idx=[0], best_dist=[2], stage=[0], n_found=1))
    # strict < (:1403): of equal distances the first in GetFeaturesInArea's order - cell column, cell row, index (cells are 10 x 10 pixels)
    tie = lambda xy, at: dict(keys=hand_keys(xy), desc=[flip(BASE[0], range(5)), flip(BASE[0], range(40, 45))], th=3, check_reprojection=False,
                              points=hand_points([pt(at[0], at[1], BASE[0])]))
    c["tie_earlier_cell_column"] = dict(tie([(106, 100), (104, 100)], (105, 100)), expect=dict(best_idx=[1], best_dist=[5], stage=[0], n_found=1))
    c["tie_earlier_cell_row"] = dict(tie([(100, 106), (100, 104)], (100, 105)), expect=dict(best_idx=[1], best_dist=[5], stage=[0], n_found=1))
    c["tie_smaller_index"] = dict(tie([(101, 101), (100, 100)], (100.5, 100.5)), expect=dict(best_idx=[0], best_dist=[5], stage=[0], n_found=1))
    # bestDist <= TH_LOW (:1411): 50 counts, 51 does not (both are reported)
    c["th_low_inclusive"] = dict(keys=hand_keys([(100, 100), (300, 300)]), desc=[flip(BASE[0], range(50)), flip(BASE[1], range(51))], th=3,
                                 points=hand_points([pt(100, 100, BASE[0]), pt(300, 300, BASE[1])]),
                                 expect=dict(best_idx=[0, 1], best_dist=[50, 51], stage=[0, 0], n_found=1))
    # bRight: the right keypoints, the descriptor rows behind the NLeft left ones, bestIdx = idx + NLeft; the left keypoint at the
    # same place carries the point's own descriptor and is never looked at
    c["right_adds_nleft"] = dict(keys=hand_keys([(300, 220), (10, 10)]), keys_right=hand_keys([(50, 50), (300, 220)]),
                                 desc=[BASE[0], BASE[1], BASE[2], flip(BASE[0], range(6))], th=3, right=True,
                                 points=hand_points([pt(300, 220, BASE[0])]), expect=dict(best_idx=[3], best_dist=[6], stage=[0], n_found=1))
    for v in c.values():
        v.setdefault("check_reprojection", True)
        v.setdefault("right", False)
        v.setdefault("uright", None)
        v.setdefault("keys_right", None)
        v.setdefault("valid", None)
    return c


def hand_target(case, gF):
    from fasttrack_amd import orb
    return dict(kf=gF, Tcw=orb.SE3(IDENTITY.q, IDENTITY.t), Ow=np.zeros(3, np.float32), log_scale_factor=LOG_SF, th=case["th"], right=case["right"],
                cam2=CAM if case["right"] else None, valid=case["valid"], check_reprojection=case["check_reprojection"])


def run_hand_case(case):
    oF, _ = hand_view(case["keys"], case["desc"], case["uright"], keys_right=case["keys_right"])
    return ref.fuse(oF, case["points"], IDENTITY, np.zeros(3, np.float32), LOG_SF, case["th"], case["right"], CAM if case["right"] else None,
                    case["valid"], case["check_reprojection"])


def cell_crowd(n_band, n_other=3):
    """One grid cell (10 x 10 pixels at (300, 220)) with n_band keypoints of octave 0 and n_other of octave 2, positions 0.03 px
    apart inside the 3-pixel box of a point aimed at the cell, descriptors 1 .. 40 bits from the point's (the nearest ones in the
    middle of the list, up to three of them: a tie the smallest index wins; the other octave's are the point's own) -> a hand case without expectation"""
    n = n_band + n_other
    xy = [(300.2 + 0.03 * (k % 17), 220.2 + 0.03 * (k // 17)) for k in range(n)]
    octave = [0] * n_band + [2] * n_other
    bits = [1 + (abs(k - n_band // 2) // 2) % 40 for k in range(n_band)] + [0] * n_other
    desc = [flip(BASE[0], range(b)) for b in bits]
    return dict(keys=hand_keys(xy, octave=octave), desc=desc, th=3, points=hand_points([(300.4, 220.4, 5.0, 0, BASE[0])]), right=False, uright=None,
                keys_right=None, valid=None, check_reprojection=True)

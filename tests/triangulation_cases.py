"""Inputs of ORBmatcher::SearchForTriangulation for the tests of ft_search_for_triangulation: geometric scenarios (3-D points in
front of posed cameras, projected into keyframe 1 and its neighbours) for the three camera forms - pinhole at 320 x 240,
KannalaBrandt8 at 256 x 256 with one camera, KannalaBrandt8 with two cameras and a Trl - and hand-built cases whose expected
outputs are written out from the reference text (src/ORBmatcher.cc:1006-1245).  Keyframes and pairs are the dicts
tests/triangulation_ref.py takes; to_device() turns them into the library's objects.

A neighbour's descriptors are keyframe-1 descriptors with a few bits flipped; the FeatureVectors come from a synthetic vocabulary
(fasttrack_amd.synth.make_vocabulary) through the oracle's transform.  Deliberate additions: distractors (a copy of the
keyframe-1 descriptor - distance 0, closer than the true match - at a position off the epipolar line: the nearest candidate
fails the constraint and the next one wins), exact duplicates of the true match in one node (the last one wins), distances of
exactly 50 and 51, forward motion with keypoints at and just inside the epipole's rejection radius, map points on both sides,
mixed mvuRight, angles with one dominant rotation and outliers.
"""
import functools

import numpy as np

from fasttrack_amd import scenarios as fsc
from fasttrack_amd import synth
from oracle import binding as ob

KP = ob.KP_DTYPE
f32 = np.float32
NLEVELS = 8
SF = ob.scale_factors(1.2, NLEVELS)[0].astype(f32)
SIGMA2 = (SF * SF).astype(f32)
PINHOLE_CAM = [262.5, 261.0, 159.5, 120.5, 0, 0, 0, 0]  # 320 x 240
KB8_CAM = [95.5, 95.4, 127.4, 128.6, 0.0034, 0.0007, -0.0020, 0.00020]  # 256 x 256
KB8_CAM2 = [96.1, 95.9, 128.9, 127.2, 0.0031, 0.0009, -0.0018, 0.00015]
FORMS = ("pinhole", "kb8", "kb8x2")
SIZE = {"pinhole": (320, 240), "kb8": (256, 256), "kb8x2": (256, 256)}


@functools.lru_cache(maxsize=None)
def vocabulary(k=6, L=3, seed=7):
    """-> (synth dict, oracle Vocabulary): no stopped words, so a FeatureVector lists every feature"""
    v = synth.make_vocabulary(k, L, seed, stop_fraction=0.0)
    return v, ob.Vocabulary(k=v["k"], L=v["L"], parent=v["parent"], is_leaf=v["is_leaf"], descriptors=v["descriptors"], weights=v["weights"])


def _rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    if th < 1e-12:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def _se3(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _project(model, cam, P):
    P = np.asarray(P, np.float64).reshape(-1, 3)
    if model == 0:
        return np.stack([cam[0] * P[:, 0] / P[:, 2] + cam[2], cam[1] * P[:, 1] / P[:, 2] + cam[3]], 1)
    return fsc.kb8_project64(cam, P)


def _flip(rng, d, nbits):
    bits = np.unpackbits(d)
    bits[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(bits)


def _keys(xy, octave, angle):
    k = np.zeros(len(xy), KP)
    if len(xy):
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        k["x"], k["y"], k["octave"], k["angle"] = xy[:, 0].astype(f32), xy[:, 1].astype(f32), octave, np.asarray(angle, f32)
        k["size"] = 31.0
    return k


def keyframe(keys, desc, fv, has_point, model, cam, cam2=None, two_cameras=False, n_left=-1, uright=None):
    return dict(keys=keys, descriptors=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), fv_nodes=np.asarray(fv["fv_nodes"], np.uint32),
                fv_offsets=np.asarray(fv["fv_offsets"], np.int32), fv_features=np.asarray(fv["fv_features"], np.uint32),
                has_point=np.asarray(has_point, np.uint8), uright=None if uright is None else np.asarray(uright, f32), n_left=n_left,
                two_cameras=bool(two_cameras), cam_model=model, cam=list(cam), cam2=list(cam if cam2 is None else cam2),
                scale_factors=SF, level_sigma2=SIGMA2)


def one_node(order, node=0):
    """a FeatureVector with a single node that lists the features in `order`"""
    order = np.asarray(order, np.uint32)
    return dict(fv_nodes=np.array([node], np.uint32), fv_offsets=np.array([0, len(order)], np.int32), fv_features=order)


def pair_constants(model, cam1, cam2, T1, T2, Trl=None, precision=1e-6):
    """The constants of (pKF1, pKF2) (:1013-1042) in float64, rounded to float32 once: T1 / T2 = T1w / T2w (4 x 4), Trl = the
    rig's left-to-right transform of two-camera keyframes (GetRightPose = Trl * Tcw)"""
    Tw2 = np.linalg.inv(T2)
    Cw = np.linalg.inv(T1)[:3, 3]
    C2 = T2[:3, :3] @ Cw + T2[:3, 3]
    with np.errstate(all="ignore"):
        ep = _project(model, cam2, C2)[0]
    poses = [T1 @ Tw2]
    if Trl is not None:
        Tr1, Twr2 = Trl @ T1, np.linalg.inv(Trl @ T2)
        poses = [T1 @ Tw2, T1 @ Twr2, Tr1 @ Tw2, Tr1 @ Twr2]  # ll, lr, rl, rr
    R = np.zeros((4, 3, 3), f32)
    t = np.zeros((4, 3), f32)
    for k, T in enumerate(poses):
        R[k], t[k] = T[:3, :3], T[:3, 3]
    F12 = np.zeros((3, 3), f32)
    if model == 0:
        K1 = np.array([[cam1[0], 0, cam1[2]], [0, cam1[1], cam1[3]], [0, 0, 1.0]])
        K2 = np.array([[cam2[0], 0, cam2[2]], [0, cam2[1], cam2[3]], [0, 0, 1.0]])
        t12 = poses[0][:3, 3]
        tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
        F12 = (np.linalg.inv(K1.T) @ tx @ poses[0][:3, :3] @ np.linalg.inv(K2)).astype(f32)
    return dict(ep=np.nan_to_num(ep).astype(f32), F12=F12, R12=R, t12=t, kb8_precision=precision)


@functools.lru_cache(maxsize=None)
def scenario(form, seed, n=300, neighbours=3, forward=False, levelsup=1, empty_neighbour=False, foreign_neighbour=False, vocab=(6, 3, 7)):
    """keyframe 1 with ~n features against `neighbours` keyframes -> dict(kf1, neighbours, pairs).  forward: the neighbours lie
    ahead of keyframe 1, so the epipole is inside the image.  empty_neighbour / foreign_neighbour: one more neighbour with no
    feature / with features of other vocabulary nodes only.  vocab: (k, L, seed) of the synthetic vocabulary."""
    rng = np.random.default_rng(seed)
    model = 0 if form == "pinhole" else 1
    two = form == "kb8x2"
    cam, cam2 = (PINHOLE_CAM, PINHOLE_CAM) if model == 0 else (KB8_CAM, KB8_CAM2 if two else KB8_CAM)
    W, H = SIZE[form]
    Trl = _se3(_rodrigues(np.array([0.004, -0.01, 0.003])), np.array([-0.11, 0.003, 0.001])) if two else None
    voc, ovoc = vocabulary(*vocab)
    leaves = voc["descriptors"][voc["is_leaf"] == 1]
    # 3-D points in front of keyframe 1 (world = its neighbourhood)
    z = rng.uniform(1.0, 3.5, n)
    span = 0.45 if model == 0 else 0.8
    Xw = np.stack([rng.uniform(-span, span, n) * z, rng.uniform(-span * 0.75, span * 0.75, n) * z, z], 1)
    T1 = _se3(_rodrigues(rng.normal(0, 0.01, 3)), rng.normal(0, 0.01, 3))
    d1 = np.stack([_flip(rng, leaves[rng.integers(0, len(leaves))], int(rng.integers(0, 21))) for _ in range(n)])
    octave = rng.integers(0, 4, n)
    a1 = rng.uniform(0, 360, n)
    right1 = (rng.random(n) < 0.4) if two else np.zeros(n, bool)

    def view(T, right):
        """pixel positions of the points in the keyframe with pose T (left or right camera per point)"""
        out = np.zeros((n, 2))
        for r, c in ((False, cam), (True, cam2)):
            Tc = (Trl @ T) if (r and two) else T
            m = right == r
            if m.any():
                P = Xw[m] @ Tc[:3, :3].T + Tc[:3, 3]
                out[m] = _project(model, c, P)
        return out

    def assemble(xy, desc, octv, ang, right, extra_has=0.12, uright_frac=None):
        """features in left-then-right order (shuffled inside each camera) -> (keyframe, position of input row i)"""
        cnt = len(xy)
        order = np.concatenate([rng.permutation(np.nonzero(~right)[0]), rng.permutation(np.nonzero(right)[0])]).astype(int)
        pos = np.empty(cnt, int)
        pos[order] = np.arange(cnt)
        keys = _keys(np.asarray(xy).reshape(-1, 2)[order], np.asarray(octv)[order], np.mod(np.asarray(ang)[order], 360.0))
        dd = np.asarray(desc, np.uint8).reshape(-1, 32)[order]
        ur = None
        if uright_frac is not None:
            ur = np.where(rng.random(cnt) < uright_frac, keys["x"] - f32(3.0), f32(-1)).astype(f32)
        kf = keyframe(keys, dd, ovoc.transform(dd, levelsup), rng.random(cnt) < extra_has, model, cam, cam2, two,
                      int((~right).sum()) if two else -1, ur)
        return kf, pos

    xy1 = view(T1, right1) + rng.normal(0, 0.3, (n, 2))
    kf1, _ = assemble(xy1, d1, octave, a1, right1, uright_frac=0.5 if form == "pinhole" else None)
    # assemble() permuted keyframe 1: keep its own arrays as the source of the neighbours' descriptors
    src_desc, src_xy_noise = d1, 0.3
    kfs, pairs = [], []
    for k in range(neighbours):
        if forward:
            t = np.array([rng.normal(0, 0.02), rng.normal(0, 0.02), -rng.uniform(0.3, 0.5)])  # T2w: the camera moved ahead
        else:
            ang = rng.uniform(0, 2 * np.pi)
            t = np.array([np.cos(ang), np.sin(ang), 0.1 * rng.normal()]) * rng.uniform(0.25, 0.4)
        T2 = _se3(_rodrigues(rng.normal(0, 0.02, 3)), t) @ T1
        right2 = (rng.random(n) < 0.4) if two else np.zeros(n, bool)
        xy2 = view(T2, right2)
        rot = rng.uniform(0, 360)
        rows_xy, rows_d, rows_o, rows_a, rows_r = [], [], [], [], []

        def add(x, d, o, a, r):
            rows_xy.append(x); rows_d.append(d); rows_o.append(o); rows_a.append(a); rows_r.append(r)

        kind = rng.random(n)
        for i in range(n):
            a2 = a1[i] - rot + (rng.uniform(0, 360) if rng.random() < 0.15 else rng.normal(0, 3))
            if kind[i] < 0.06:        # exactly 50 / 51 bits from keyframe 1, no other candidate of this point
                add(xy2[i], _flip(rng, src_desc[i], 50 if kind[i] < 0.03 else 51), octave[i], a2, right2[i])
                continue
            if kind[i] < 0.12:        # no match in this neighbour
                continue
            true_d = _flip(rng, src_desc[i], int(rng.integers(1, 9)))
            add(xy2[i] + rng.normal(0, src_xy_noise, 2), true_d, octave[i], a2, right2[i])
            if kind[i] < 0.30:        # distractor: distance 0 at a position off the epipolar line
                add(np.array([rng.uniform(20, W - 20), rng.uniform(20, H - 20)]), src_desc[i].copy(), octave[i], a2, right2[i])
            elif kind[i] < 0.42:      # exact duplicates of the true match: the last of the node's list wins
                for _ in range(int(rng.integers(1, 3))):
                    add(rows_xy[-1].copy(), true_d.copy(), octave[i], a2, right2[i])
        if forward and model == 0:    # keypoints around the epipole: inside, just inside, just outside its rejection radius
            pc = pair_constants(model, cam, cam, T1, T2)
            for j in range(24):
                o = int(rng.integers(0, 4))
                rad = np.sqrt(100.0 * float(SF[o])) * [0.4, 0.97, 0.999, 1.001, 1.03, 1.5][j % 6]
                th = rng.uniform(0, 2 * np.pi)
                i = int(rng.integers(0, n))
                add(pc["ep"].astype(np.float64) + rad * np.array([np.cos(th), np.sin(th)]), _flip(rng, src_desc[i], int(rng.integers(0, 4))), o,
                    a1[i] - rot, False)
        for _ in range(n // 10):      # unrelated features
            add(np.array([rng.uniform(20, W - 20), rng.uniform(20, H - 20)]), rng.integers(0, 256, 32, dtype=np.uint8), int(rng.integers(0, 4)),
                rng.uniform(0, 360), bool(two and rng.random() < 0.4))
        kf2, _ = assemble(np.array(rows_xy), np.array(rows_d), np.array(rows_o), np.array(rows_a), np.array(rows_r, bool),
                          uright_frac=0.5 if form == "pinhole" else None)
        kfs.append(kf2)
        pairs.append(pair_constants(model, cam, cam, T1, T2, Trl))
    if empty_neighbour:
        kfs.insert(1, keyframe(_keys([], [], []), np.zeros((0, 32), np.uint8), dict(fv_nodes=[], fv_offsets=[0], fv_features=[]), [], model,
                               cam, cam2, two, 0 if two else -1))
        pairs.insert(1, pairs[0])
    if foreign_neighbour:
        kfs.append(dict(kfs[0], fv_nodes=(np.asarray(kfs[0]["fv_nodes"]) + np.uint32(100000)).astype(np.uint32)))
        pairs.append(pairs[0])
    return dict(kf1=kf1, neighbours=kfs, pairs=pairs)


# the scenarios the CPU and the GPU tests share: (form, seed, forward); seeds chosen so that the restatement reports, over the
# set, every order-dependent event (test_triangulation_cpu.py asserts it)
MAIN = [("pinhole", 11, False), ("pinhole", 12, True), ("kb8", 13, False), ("kb8x2", 14, False)]


def node_size_case(form, size, seed):
    """everything in ONE node (levelsup >= L): keyframe 1 with 40 features against a neighbour with `size` candidates"""
    S = scenario(form, seed, n=40, neighbours=1, levelsup=3)
    kf2 = S["neighbours"][0]
    n2 = len(kf2["keys"])
    reps = -(-size // n2)
    idx = np.tile(np.arange(n2), reps)[:size]
    if form == "kb8x2":  # keep left features in front of right ones
        idx = np.concatenate([idx[idx < kf2["n_left"]], idx[idx >= kf2["n_left"]]])
    nl = int((idx < kf2["n_left"]).sum()) if form == "kb8x2" else -1
    dd = kf2["descriptors"][idx]
    k2 = keyframe(kf2["keys"][idx], dd, vocabulary()[1].transform(dd, 3), kf2["has_point"][idx], kf2["cam_model"], kf2["cam"], kf2["cam2"],
                  kf2["two_cameras"], nl, None if kf2["uright"] is None else kf2["uright"][idx])
    return dict(kf1=S["kf1"], neighbours=[k2], pairs=S["pairs"])


# ---- hand-built cases ---------------------------------------------------------------------------------------------------------
# Pinhole with K = identity-like intrinsics folded into F12 = hat((1, 0, 0)): a = 0, b = 1, c = -y1, so num = y2 - y1, den = 1 and
# the constraint is (y2 - y1)^2 < 3.84 sigma2: a candidate on the row of its feature passes, one 3 px off at level 0 does not.
F_ROWS = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)
FAR_EP = (-1000.0, -1000.0)


def _hand_pair(ep=FAR_EP, F12=F_ROWS):
    return dict(ep=np.asarray(ep, f32), F12=np.asarray(F12, f32), R12=np.tile(np.eye(3, dtype=f32), (4, 1, 1)), t12=np.zeros((4, 3), f32),
                kb8_precision=1e-6)


def _hand_kf(xy, desc, order=None, octave=None, angle=None, has_point=None, uright=None, model=0, two=False, n_left=-1):
    n = len(xy)
    keys = _keys(np.asarray(xy, np.float64).reshape(-1, 2), np.zeros(n, int) if octave is None else octave, np.zeros(n) if angle is None else angle)
    return keyframe(keys, np.asarray(desc, np.uint8).reshape(-1, 32), one_node(np.arange(n) if order is None else order),
                    np.zeros(n, np.uint8) if has_point is None else has_point, model, KB8_CAM if model else PINHOLE_CAM,
                    KB8_CAM2 if two else None, two, n_left, uright)


def hand_built():
    """-> list of dict(name, kf1, kf2, pair, flags = (only_stereo, coarse, check_orientation), matches12, n, best_dist): the
    expected outputs are written out from the reference text, not computed"""
    rng = np.random.default_rng(2024)
    D = rng.integers(0, 256, (40, 32), dtype=np.uint8)  # unrelated descriptors: pairwise distances around 128
    out = []

    def case(name, kf1, kf2, pair, flags, matches12, n, best_dist):
        out.append(dict(name=name, kf1=kf1, kf2=kf2, pair=pair, flags=flags, matches12=np.asarray(matches12, np.int32), n=n,
                        best_dist=np.asarray(best_dist, np.int32)))

    # equal distances: the LAST of the node's list wins (list order 2, 0, 1 -> feature 1)
    case("tie_goes_to_the_last", _hand_kf([[50, 60]], [D[0]]), _hand_kf([[80, 60], [90, 60], [70, 60]], [D[0]] * 3, order=[2, 0, 1]),
         _hand_pair(), (False, False, False), [1], 1, [0])
    # dist == 50 is accepted, 51 is not
    case("th_low_50_and_51", _hand_kf([[50, 60], [50, 90]], [D[0], D[1]]),
         _hand_kf([[80, 60], [80, 90]], [_flip(rng, D[0], 50), _flip(rng, D[1], 51)]), _hand_pair(), (False, False, False), [0, -1], 1, [50, 50])
    # the epipole comparison is strict: 6^2 + 8^2 = 100 is not < 100 * 1.0 (level 0), 6^2 + 7.5^2 is
    case("epipole_is_strict", _hand_kf([[50, 108], [50, 107.5]], [D[0], D[1]]), _hand_kf([[106, 108], [106, 107.5]], [D[0], D[1]]),
         _hand_pair(ep=(100, 100)), (False, False, False), [0, -1], 1, [0, 50])
    # ... and does not apply to a stereo feature (bStereo2)
    case("epipole_not_for_stereo", _hand_kf([[50, 107.5]], [D[1]]), _hand_kf([[106, 107.5]], [D[1]], uright=[100.0]),
         _hand_pair(ep=(100, 100)), (False, False, False), [0], 1, [0])
    # den == 0 rejects (F12 = 0), bCoarse skips the constraint
    case("den_zero_rejects", _hand_kf([[50, 60]], [D[0]]), _hand_kf([[80, 60]], [D[0]]), _hand_pair(F12=np.zeros((3, 3))),
         (False, False, False), [-1], 0, [50])
    case("coarse_skips_the_constraint", _hand_kf([[50, 60]], [D[0]]), _hand_kf([[80, 60]], [D[0]]), _hand_pair(F12=np.zeros((3, 3))),
         (False, True, False), [0], 1, [0])
    # ... but not the epipole test: candidate 0 lies 5 px from the epipole, candidate 1 (distance 3) is taken
    case("coarse_keeps_the_epipole_test", _hand_kf([[50, 60]], [D[0]]), _hand_kf([[105, 100], [200, 60]], [D[0], _flip(rng, D[0], 3)]),
         _hand_pair(ep=(100, 100), F12=np.zeros((3, 3))), (False, True, False), [1], 1, [3])
    # the nearest candidate fails the constraint (3 px off the row), the next one wins with its larger distance
    case("constraint_rejects_the_nearest", _hand_kf([[50, 60]], [D[0]]), _hand_kf([[80, 63], [90, 60]], [D[0], _flip(rng, D[0], 7)]),
         _hand_pair(), (False, False, False), [1], 1, [7])
    # bOnlyStereo with two cameras matches nothing, whatever mvuRight holds (bStereo = !mpCamera2 && ...)
    case("only_stereo_with_two_cameras", _hand_kf([[100, 100], [120, 100]], [D[0], D[1]], uright=[90.0, 110.0], model=1, two=True, n_left=1),
         _hand_kf([[101, 100], [121, 100]], [D[0], D[1]], uright=[91.0, 111.0], model=1, two=True, n_left=1), _hand_pair(),
         (True, True, False), [-1, -1], 0, [50, 50])
    # bOnlyStereo with one camera: only features with mvuRight >= 0 on both sides
    case("only_stereo_one_camera", _hand_kf([[50, 60], [50, 90], [50, 120]], D[:3], uright=[40.0, -1.0, 45.0]),
         _hand_kf([[80, 60], [80, 90], [80, 120]], D[:3], uright=[70.0, 75.0, -1.0]), _hand_pair(), (True, False, False), [0, -1, -1], 1,
         [0, 50, 50])
    # a keyframe-1 feature with a map point is skipped; a candidate with one is not eligible
    case("map_points_on_both_sides", _hand_kf([[50, 60], [50, 90], [50, 120]], D[:3], has_point=[1, 0, 0]),
         _hand_kf([[80, 60], [80, 90], [80, 120]], D[:3], has_point=[0, 1, 0]), _hand_pair(), (False, False, False), [-1, -1, 2], 1, [50, 50, 0])
    # the histogram removes exactly the bins that are not among the three largest: sizes 10, 6, 4, 2, 1 in bins 0, 5, 9, 12, 20
    bins = [0] * 10 + [5] * 6 + [9] * 4 + [12] * 2 + [20]
    nb = len(bins)
    xy = [[20 + 10 * i, 30 + 8 * i] for i in range(nb)]
    case("histogram_keeps_three_bins", _hand_kf(xy, D[:nb], angle=[30.0 * b for b in bins]), _hand_kf(xy, D[:nb]), _hand_pair(),
         (False, True, True), [i if bins[i] in (0, 5, 9) else -1 for i in range(nb)], 20, [0] * nb)
    # ... and nothing without mbCheckOrientation
    case("no_orientation_check", _hand_kf(xy, D[:nb], angle=[30.0 * b for b in bins]), _hand_kf(xy, D[:nb]), _hand_pair(),
         (False, True, False), list(range(nb)), nb, [0] * nb)
    return out


def rotation_cases():
    """the directed histograms of the rotation filter (bow_kf_cases.rotation_table) -> list of dict(name, kf1, neighbours, pairs,
    flags, matches12 [J, n1], n [J], best_dist [J, n1]): one per histogram, and `rotation_all_in_one_call` (filter on and off) with
    every histogram as a neighbour of the SAME keyframe 1.  All features share one node; the descriptors are unrelated (pairwise
    distances far above TH_LOW), a neighbour's are copies of keyframe 1's first ones, so feature i matches its copy at distance 0
    (bCoarse: no constraint) and the features beyond a neighbour's nothing.  Keyframe 1's angles are 0, a neighbour's minus its
    matches' rotations (kp1.angle - kp2.angle, :1188)."""
    from tests import bow_kf_cases as bk
    table = bk.rotation_table()
    out = []

    def case(name, n1, rots, ori):
        d = bk.angles_decide(np.zeros(n1), [])[0]
        xy = [[20 + 10 * i, 30 + 8 * i] for i in range(n1)]
        nbs, want, best = [], np.full((len(rots), n1), -1, np.int32), np.full((len(rots), n1), 50, np.int32)
        for k, (rot, kept) in enumerate(rots):
            n = len(rot)
            nbs.append(_hand_kf(xy[:n], d[:n], angle=-rot))
            hit = np.nonzero(kept | (not ori))[0]
            want[k, hit] = hit
            best[k, :n] = 0  # bestDist of a match the histogram removes stays
        out.append(dict(name=name, kf1=_hand_kf(xy, d), neighbours=nbs, pairs=[_hand_pair() for _ in rots], flags=(False, True, ori),
                        matches12=want, n=(want >= 0).sum(axis=1).astype(np.int32), best_dist=best))

    for name, rot, kept, _ in table:
        case("rotation_" + name, max(len(rot), 1), [(rot, kept)], True)
    n1 = max(len(rot) for _, rot, _, _ in table)
    for ori in (True, False):
        case("rotation_all_in_one_call" + ("" if ori else "_filter_off"), n1, [(rot, kept) for _, rot, kept, _ in table], ori)
    return out


def four_pairings():
    """two-camera keyframes with one left and one right feature each, all four with the same descriptor in one node, and four
    distinguishable poses -> (kf1, kf2, pair)"""
    rng = np.random.default_rng(5)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    kf1 = _hand_kf([[100, 110], [140, 120]], [d, d], model=1, two=True, n_left=1)
    kf2 = _hand_kf([[104, 111], [143, 118]], [d, d], model=1, two=True, n_left=1)
    P = _hand_pair()
    for k in range(4):
        P["R12"][k] = _rodrigues(np.array([0.01 * (k + 1), -0.02 * (k + 1), 0.005 * (k + 1)])).astype(f32)
        P["t12"][k] = np.array([0.1 * (k + 1), 0.01 * k, -0.02 * k], f32)
    return kf1, kf2, P


def to_device(orb, kf):
    """a keyframe dict as the library's TriangKeyFrame"""
    return orb.TriangKeyFrame(kf["keys"], kf["descriptors"], kf["fv_nodes"], kf["fv_offsets"], kf["fv_features"], kf["has_point"],
                              kf["scale_factors"], kf["level_sigma2"], kf["cam"], kf["cam2"], kf["cam_model"], kf["two_cameras"], kf["n_left"],
                              kf["uright"])


def to_device_pair(orb, p):
    two = np.any(np.asarray(p["R12"])[1:] != 0)
    R, t = np.asarray(p["R12"], f32), np.asarray(p["t12"], f32)
    return orb.make_triang_pair(p["ep"], p["F12"], R if two else R[:1], t if two else t[:1], p["kb8_precision"])

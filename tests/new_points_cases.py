"""Inputs of the triangulation loop of LocalMapping::CreateNewMapPoints for the tests of ft_triangulate_new_points /
ft_search_and_triangulate: geometric scenarios for the three camera forms of tests/triangulation_cases.py (known 3-D points, posed
keyframes, pixel noise, match rows that mix true correspondences, wrong ones and pairs pushed across the thresholds), directed
hand-built cases with the status the reference text (src/LocalMapping.cc:483-692) gives them, and rows with a chosen number of
matches for the compaction of the kernel.  Keyframes are the dicts of tests/triangulation_ref.py, geometries the dicts of
tests/new_points_ref.py; to_device_geometry() turns the latter into the library's objects.

The stand-alone stage reads neither descriptors nor FeatureVectors: the keyframes built here carry zeros / an empty vector.
"""
import functools

import numpy as np

from tests import new_points_ref as npr
from tests import triangulation_cases as tc

f32 = np.float32
FORMS = tc.FORMS
RATIO_FACTOR = float(f32(1.5) * f32(1.2))  # 1.5f * mfScaleFactor
MB = 0.12                                  # stereo baseline of the pinhole form [m]
MBF = float(f32(tc.PINHOLE_CAM[0]) * f32(MB))
CHUNK = 256                                # slots of a k_triang_points workgroup

# Tolerances of test_new_points_cpu.py, MEASURED over exact_cases() and multiplied by 4, as relative errors |a - b| / |b|:
#   NULLVEC_TOL  x3D of the restated null_vector4 against x3D of np.linalg.svd (float64) on the same matrix A: 3.58e-14 observed
#   TRUTH_TOL    an accepted x3D against the ground-truth point: 3.61e-6 observed.  Keypoints and poses are narrowed to float32
#                before A is formed, which neither SVD sees: the float64 SVD of the same A is off the truth by 3.62e-6 itself
NULLVEC_TOL = 4 * 3.58e-14
TRUTH_TOL = 4 * 3.62e-6

# Whether every status is reachable.  -2 through Triangulate needs the fourth component of the null vector to be exactly 0 after
# narrowing to float (|w| < 2^-150 in double, with |v| = 1), i.e. a point at infinity: parallel rays from two centres.  Parallel
# rays have cosParallaxRays == 1 up to one rounding, and the branch that calls Triangulate wants cosParallaxRays < cosParallaxStereo
# <= 1: only a stereo keypoint whose cosParallaxStereo rounds to 1.0f while the rays' cosine rounds below it gets there, and then
# the rays are not along the optical axis, the columns of A are coupled and the rotations leave w a sum of products of order
# 1e-17, not 0.  The exactly decoupled system (both keypoints at the principal point, w == 0 exactly) has cosParallaxRays == 1 and
# never reaches Triangulate.  So it is not forced: -2 is reached through UnprojectStereo (depth <= 0) only.
# -7 (a zero distance) is unreachable with a camera centre that belongs to the pose:
# x3D == Ow gives z == 0, which -3 / -4 reject first; the directed case hands the library an Ow that is the stereo point itself.
REACHABLE = (0, 1, 2, 3, -1, -2, -3, -4, -5, -6, -7, -8, -9)


def _empty_fv():
    return dict(fv_nodes=[], fv_offsets=[0], fv_features=[])


def _keyframe(keys, model, cam, cam2=None, two=False, n_left=-1, uright=None):
    n = len(keys)
    return tc.keyframe(keys, np.zeros((n, 32), np.uint8), _empty_fv(), np.zeros(n, np.uint8), model, cam, cam2, two, n_left, uright)


def geometry(T, cam, Trl=None, mb=0.0, mbf=0.0, depth=None, keys_raw=None, precision=1e-6):
    """the geometry dict of a keyframe with pose T = Tcw (4 x 4, float64); Trl: the rig's left-to-right transform"""
    T = np.asarray(T, np.float64)
    Tr = T if Trl is None else Trl @ T
    fx, fy = f32(cam[0]), f32(cam[1])
    return dict(Tcw=T[:3].astype(f32), Ow=np.linalg.inv(T)[:3, 3].astype(f32), Tcw_right=Tr[:3].astype(f32),
                Ow_right=np.linalg.inv(Tr)[:3, 3].astype(f32), Rwc=T[:3, :3].T.astype(f32), twc=np.linalg.inv(T)[:3, 3].astype(f32),
                fx=fx, fy=fy, cx=f32(cam[2]), cy=f32(cam[3]), invfx=f32(f32(1) / fx), invfy=f32(f32(1) / fy), mb=f32(mb), mbf=f32(mbf),
                depth=None if depth is None else np.asarray(depth, f32), keys_raw=keys_raw, kb8_precision=precision)


def geometry_from_pair(kf, pair, first):
    """geometry of the keyframes of a tests/triangulation_cases.py scenario: keyframe 1 is the world (first), a neighbour is posed
    by the pair's T12 = T1w * Tw2; two-camera keyframes get the Trl the four pairings imply"""
    R, t = np.asarray(pair["R12"], np.float64), np.asarray(pair["t12"], np.float64)
    T12 = tc._se3(R[0], t[0])
    Trl = tc._se3(R[2], t[2]) @ np.linalg.inv(T12) if kf["two_cameras"] else None
    n = len(kf["keys"])
    depth = None
    if kf["uright"] is not None:  # mvDepth = mbf / disparity (src/Frame.cc:1000-1006)
        with np.errstate(all="ignore"):
            depth = np.where(kf["uright"] >= 0, f32(MBF) / (kf["keys"]["x"] - kf["uright"]).astype(f32), f32(-1)).astype(f32)
    assert depth is None or len(depth) == n
    return geometry(np.eye(4) if first else np.linalg.inv(T12), kf["cam"], Trl, MB, MBF, depth)


@functools.lru_cache(maxsize=None)
def scenario(form, seed, n1=200, neighbours=3, exact=False):
    """-> dict(kf1, g1, neighbours, geometries, matches12 [k, n1], truth [n1, 3], true_match [k, n1] bool).  exact: no noise, true
    correspondences only, nothing pushed across a threshold - an accepted point is the ground truth"""
    rng = np.random.default_rng(seed)
    model = 0 if form == "pinhole" else 1
    two = form == "kb8x2"
    cam, cam2 = (tc.PINHOLE_CAM, tc.PINHOLE_CAM) if model == 0 else (tc.KB8_CAM, tc.KB8_CAM2 if two else tc.KB8_CAM)
    W, H = tc.SIZE[form]
    Trl = tc._se3(tc._rodrigues(np.array([0.004, -0.01, 0.003])), np.array([-0.11, 0.003, 0.001])) if two else None
    noise = 0.0 if exact else 0.3
    z = rng.uniform(1.0, 3.5, n1)
    if not exact:
        z = np.where(rng.random(n1) < 0.08, z * 60, z)  # far points: parallax below the 0.9998 / 0.9996 limits
    span = 0.45 if model == 0 else 0.8
    Xw = np.stack([rng.uniform(-span, span, n1) * z, rng.uniform(-span * 0.75, span * 0.75, n1) * z, z], 1)
    T1 = tc._se3(tc._rodrigues(rng.normal(0, 0.01, 3)), rng.normal(0, 0.01, 3))
    octave = rng.integers(0, 4, n1)

    def view(T, right):
        """-> pixel positions and depths of the points in the keyframe with pose T (left or right camera per point)"""
        out, depth = np.zeros((n1, 2)), np.zeros(n1)
        for r, c in ((False, cam), (True, cam2)):
            Tc = (Trl @ T) if (r and two) else T
            m = right == r
            if m.any():
                P = Xw[m] @ Tc[:3, :3].T + Tc[:3, 3]
                out[m], depth[m] = tc._project(model, c, P), P[:, 2]
        return out, depth

    def assemble(xy, octv, right, depth):
        """features in left-then-right order (shuffled inside each camera) -> (keyframe, uright-free geometry inputs, position of row i)"""
        cnt = len(xy)
        order = np.concatenate([rng.permutation(np.nonzero(~right)[0]), rng.permutation(np.nonzero(right)[0])]).astype(int)
        pos = np.empty(cnt, int)
        pos[order] = np.arange(cnt)
        keys = tc._keys(np.asarray(xy).reshape(-1, 2)[order], np.asarray(octv)[order], np.zeros(cnt))
        ur = dep = raw = None
        if model == 0:  # stereo keypoints with mvuRight / mvDepth; mvKeys off mvKeysUn by a smooth fraction of a pixel
            d = np.asarray(depth)[order]
            stereo = (rng.random(cnt) < 0.5) & (d > 0)
            with np.errstate(all="ignore"):
                ur = np.where(stereo, keys["x"] - (MBF / d).astype(f32) + rng.normal(0, noise / 2, cnt).astype(f32), f32(-1)).astype(f32)
            ur = np.where(stereo & (ur < 0), f32(0), ur).astype(f32)
            dep = np.where(stereo, d, -1).astype(f32)
            raw = keys.copy()
            if not exact:
                raw["x"] = (keys["x"] + f32(0.4) * np.sin(keys["y"] / f32(40))).astype(f32)
                raw["y"] = (keys["y"] + f32(0.4) * np.cos(keys["x"] / f32(50))).astype(f32)
        kf = _keyframe(keys, model, cam, cam2, two, int((~right).sum()) if two else -1, ur)
        return kf, dep, raw, pos

    right1 = (rng.random(n1) < 0.4) if two else np.zeros(n1, bool)
    xy1, d1 = view(T1, right1)
    kf1, dep1, raw1, pos1 = assemble(xy1 + rng.normal(0, noise, (n1, 2)), octave, right1, d1)
    g1 = geometry(T1, cam, Trl, MB, MBF, dep1, raw1)
    kfs, geos = [], []
    m12 = np.full((neighbours, n1), -1, np.int32)
    true_match = np.zeros((neighbours, n1), bool)
    for k in range(neighbours):
        ang = rng.uniform(0, 2 * np.pi)
        # the pinhole form's second neighbour sits closer than the stereo baseline: its stereo keypoints give stereo points
        base = 0.05 if (model == 0 and k == 1) else rng.uniform(0.25, 0.4)
        t = np.array([np.cos(ang), np.sin(ang), 0.1 * rng.normal()]) * base
        T2 = tc._se3(tc._rodrigues(rng.normal(0, 0.02, 3)), t) @ T1
        right2 = (rng.random(n1) < 0.4) if two else np.zeros(n1, bool)
        xy2, d2 = view(T2, right2)
        present = np.ones(n1, bool) if exact else rng.random(n1) < 0.75
        src = np.nonzero(present)[0]
        extra = 0 if exact else n1 // 10
        xy = np.concatenate([xy2[src] + rng.normal(0, noise, (len(src), 2)), np.stack([rng.uniform(20, W - 20, extra), rng.uniform(20, H - 20, extra)], 1)])
        octv = np.concatenate([octave[src], rng.integers(0, 4, extra)])
        if not exact:
            kind = rng.random(len(src))
            octv[:len(src)] = np.where(kind < 0.06, octv[:len(src)] + 4, octv[:len(src)])          # scale inconsistency
            push = (kind >= 0.06) & (kind < 0.14)                                                  # around the chi-square limits
            th = rng.uniform(0, 2 * np.pi, len(src))
            rad = rng.uniform(1.5, 5.0, len(src)) * np.sqrt(tc.SIGMA2[octave[src]])
            xy[:len(src)] += np.where(push[:, None], np.stack([np.cos(th), np.sin(th)], 1) * rad[:, None], 0)
        rgt = np.concatenate([right2[src], (rng.random(extra) < 0.4) if two else np.zeros(extra, bool)])
        dep = np.concatenate([d2[src], np.full(extra, 2.0)])
        kf2, dep2, raw2, pos2 = assemble(xy, octv, rgt, dep)
        kfs.append(kf2)
        geos.append(geometry(T2, cam, Trl, MB, MBF, dep2, raw2))
        where = np.full(n1, -1)
        where[src] = pos2[:len(src)]
        for i in range(n1):
            u = rng.random()
            if exact or (where[i] >= 0 and u < 0.85):
                m12[k, pos1[i]], true_match[k, pos1[i]] = where[i], where[i] >= 0
            elif u < 0.95 and (where[i] >= 0 or u < 0.88):
                m12[k, pos1[i]] = rng.integers(0, len(kf2["keys"]))  # a wrong correspondence
    truth = np.zeros((n1, 3))
    truth[pos1] = Xw
    return dict(kf1=kf1, g1=g1, neighbours=kfs, geometries=geos, matches12=m12, truth=truth, true_match=true_match,
                params=dict(inertial=False, far_points=True, th_far=150.0, ratio_factor=RATIO_FACTOR))


# the scenarios the CPU and the GPU tests share: (form, seed, n1, neighbours); seeds chosen so that every neighbour has a status 1
# and the pinhole one yields 2 and 3 (test_new_points_cpu.py asserts it)
MAIN = [("pinhole", 41, 230, 3), ("kb8", 42, 170, 2), ("kb8x2", 43, 300, 3), ("pinhole", 44, 130, 1)]


def exact_cases():
    """exact projections of known points, for the tolerances above"""
    return [scenario(form, 50 + i, n1=60, neighbours=2, exact=True) for i, form in enumerate(FORMS)]


# ---- rows with a chosen number of matches -----------------------------------------------------------------------------------------
COUNTS = (0, 1, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def boundary_base(form):
    """one neighbour that holds a true match for every one of 600 features (three chunks: 256, 256, 88)"""
    return scenario(form, 60, n1=600, neighbours=1, exact=True)


def boundary_rows(form):
    """-> the scenario and, per neighbour count case, a row [600] cut out of its full row: a status depends on its own pair only, so
    the reference of a cut row is the cut of the full reference.  The matches sit in different chunks and straddle their borders:
    1 at the last slot of the row; 63 / 64 / 65 from slot 224 on (the fourth wave of chunk 0 and the first of chunk 1); 257 from
    slot 255 on (one in chunk 0, ALL of chunk 1: no empty slot in a workgroup); and 0."""
    S = boundary_base(form)
    full = S["matches12"][0]
    rows = {}
    for c in COUNTS:
        row = np.full_like(full, -1)
        lo = {0: 0, 1: len(full) - 1, 257: CHUNK - 1}.get(c, 224)
        row[lo:lo + c] = full[lo:lo + c]
        assert int((row >= 0).sum()) == c
        rows[c] = row
    return S, rows


# ---- hand-built cases --------------------------------------------------------------------------------------------------------------
def _px(cam, P):
    return tc._project(0, cam, np.asarray(P, np.float64).reshape(1, 3))[0]


def hand_built():
    """-> list of dict(name, kf1, g1, kf2, g2, matches12, params, status): pinhole keyframes, keyframe 1 at the origin, keyframe 2
    displaced along x by `b` (or as stated).  The expected status of every feature is written out from the reference text; the
    restatement is asserted to give it (test_new_points_cpu.py) and the device to give what the restatement gives."""
    cam = tc.PINHOLE_CAM
    out = []

    def shifted(b, z=0.0):
        return tc._se3(np.eye(3), np.array([-b, 0.0, -z]))  # Tcw of a camera at (b, 0, z) looking along +z

    def case(name, T2, rows, status, mb2=MB, mbf2=MBF, mbf1=MBF, inertial=False, far_points=False, th_far=0.0, ow1=None, swap=False):
        """rows: per feature dict(X, stereo1, stereo2, depth1, depth2, o1, o2, dxy1, dxy2) - X the world point both keypoints show"""
        T1 = np.eye(4)
        k1, k2, u1, u2, dp1, dp2 = [], [], [], [], [], []
        for r in rows:
            X = np.asarray(r["X"], np.float64)
            X2 = T2[:3, :3] @ X + T2[:3, 3]
            a, b_ = _px(cam, X) + np.asarray(r.get("dxy1", (0, 0))), _px(cam, X2) + np.asarray(r.get("dxy2", (0, 0)))
            if r.get("swap"):
                a, b_ = b_, a
            k1.append(a); k2.append(b_)
            d1, d2 = r.get("depth1", X[2]), r.get("depth2", X2[2])
            dp1.append(d1 if r.get("stereo1") else -1.0); dp2.append(d2 if r.get("stereo2") else -1.0)
            u1.append(a[0] - mbf1 / X[2] if r.get("stereo1") else -1.0)
            u2.append(b_[0] - r.get("mbf_ur2", mbf2) / X2[2] if r.get("stereo2") else -1.0)
        n = len(rows)
        kf1 = _keyframe(tc._keys(k1, [r.get("o1", 0) for r in rows], np.zeros(n)), 0, cam, uright=u1)
        kf2 = _keyframe(tc._keys(k2, [r.get("o2", 0) for r in rows], np.zeros(n)), 0, cam, uright=u2)
        g1 = geometry(T1, cam, None, MB, mbf1, dp1)
        g2 = geometry(T2, cam, None, mb2, mbf2, dp2)
        if ow1 is not None:
            g1["Ow"] = np.asarray(ow1(kf1, g1), f32)
        out.append(dict(name=name, kf1=kf1, g1=g1, kf2=kf2, g2=g2, matches12=np.arange(n, dtype=np.int32).reshape(1, n),
                        params=dict(inertial=inertial, far_points=far_points, th_far=th_far, ratio_factor=RATIO_FACTOR),
                        status=np.asarray(status, np.int32)))

    X = (0.1, 0.05, 2.0)
    wide, near = shifted(0.3), shifted(0.05)  # parallax of X: 8.6 degrees; 1.4 degrees, below the stereo parallax 2 atan(0.06 / 2) = 3.4
    # 1: exact projections, parallax above every limit
    case("triangulated", wide, [dict(X=X)], [1])
    # 2 / 3: the neighbour is closer than the stereo baseline, so cosParallaxRays >= cosParallaxStereo: the stereo point of the
    # keyframe that has one (:589-600)
    case("stereo_point_of_keyframe_1", near, [dict(X=X, stereo1=True)], [2])
    case("stereo_point_of_keyframe_2", near, [dict(X=X, stereo2=True)], [3])
    # both stereo: `else if` (:571) leaves cosParallaxStereo2 at cosParallaxRays + 1, so keyframe 1's point is taken although
    # keyframe 2's baseline (mb 0.5) would give the smaller cosine (its mvuRight fits keyframe 1's mbf: see :665 below)
    case("both_stereo_else_if", near, [dict(X=X, stereo1=True, stereo2=True, mbf_ur2=MBF)], [2], mb2=0.5, mbf2=float(f32(cam[0]) * f32(0.5)))
    # -1: 30 m away over a 0.3 m baseline: cos = 0.99995, no stereo
    case("low_parallax", wide, [dict(X=(0.5, 0.2, 30.0))], [-1])
    # -2: UnprojectStereo with depth <= 0 (cosParallaxStereo1 = cos(2 atan2(0.06, -1)) = cos(0.12) = 0.993 < cosParallaxRays)
    case("unproject_stereo_fails", near, [dict(X=X, stereo1=True, depth1=-1.0), dict(X=X, stereo1=True, depth1=0.0)], [-2, -2])
    # -3: the keypoints swapped, the rays diverge: the algebraic solution lies behind both cameras
    case("behind_keyframe_1", wide, [dict(X=X, swap=True)], [-3])
    # -4: keyframe 2 stands 3 m behind the point and looks the same way: its keypoint is the image of a point BEHIND it, the
    # algebraic solution is X itself, z1 = 2, z2 = -3
    case("behind_keyframe_2", shifted(0.3, 5.0), [dict(X=X)], [-4])
    # -5: keyframe 1's keypoint 8 px off the epipolar line (level 0: 5.991 px^2)
    case("reprojection_1", wide, [dict(X=X, dxy1=(0, 8))], [-5])
    # -6: the same offset in keyframe 2 while keyframe 1's keypoint is of level 3 (sigma2 = 2.99: its half of the offset, 16 px^2,
    # stays below 5.991 * 2.99)
    case("reprojection_2", wide, [dict(X=X, dxy2=(0, 8), o1=3)], [-6])
    # :665: keyframe 2's u_r is tested with KEYFRAME 1's mbf.  Its mvuRight belongs to its own mbf (twice keyframe 1's): -6; an
    # mvuRight that fits keyframe 1's mbf passes
    mbf2 = float(f32(cam[0]) * f32(0.24))
    case("mbf_of_keyframe_1_in_test_2", wide, [dict(X=X, stereo2=True), dict(X=X, stereo2=True, mbf_ur2=MBF)], [-6, 1], mb2=0.24, mbf2=mbf2)
    # -7: only with a camera centre that is not the pose's (see REACHABLE): Ow1 = the stereo point itself
    case("zero_distance", near, [dict(X=X, stereo1=True)], [-7], ow1=lambda kf, g: npr.unproject_stereo(kf, g, 0))
    # -8: mbFarPoints with mThFarPoints = 1.5 m; without it the point is accepted
    case("far_point", wide, [dict(X=X)], [-8], far_points=True, th_far=1.5)
    case("far_points_off", wide, [dict(X=X)], [1], far_points=False, th_far=1.5)
    # -9: levels 0 and 4: ratioOctave = 1 / 1.2^4 = 0.48, ratioDist ~ 1 > 0.48 * 1.8
    case("scale_inconsistency", wide, [dict(X=X, o2=4), dict(X=X, o1=4)], [-9, -9])
    # 0.9996 (inertial) / 0.9998: 12.25 m over 0.3 m gives cos = 0.9997
    Xm = (0.0, 0.0, 12.25)
    case("between_the_limits_inertial", wide, [dict(X=Xm)], [-1], inertial=True)
    case("between_the_limits_not_inertial", wide, [dict(X=Xm)], [1], inertial=False)
    return out


def four_pairings():
    """two-camera KannalaBrandt8 keyframes with two left and two right features; the four matches are the pairings ll, lr, rl, rr of
    one world point each -> dict as hand_built() plus pairings (what new_points_ref reports must equal it)"""
    cam, cam2 = tc.KB8_CAM, tc.KB8_CAM2
    Trl = tc._se3(tc._rodrigues(np.array([0.004, -0.01, 0.003])), np.array([-0.11, 0.003, 0.001]))
    T1, T2 = np.eye(4), tc._se3(tc._rodrigues(np.array([0.01, -0.02, 0.005])), np.array([-0.3, 0.02, 0.01]))
    pts = np.array([[0.2, 0.1, 2.0], [-0.3, 0.2, 2.5], [0.4, -0.2, 1.8], [-0.1, -0.3, 2.2]])
    pairing = [0, 1, 2, 3]  # ll, lr, rl, rr

    def px(T, right, X):
        Tc = Trl @ T if right else T
        return tc._project(1, cam2 if right else cam, (Tc[:3, :3] @ X + Tc[:3, 3]).reshape(1, 3))[0]

    r1 = [p >= 2 for p in pairing]
    r2 = [p % 2 == 1 for p in pairing]
    k1 = [px(T1, r1[i], pts[i]) for i in range(4)]           # features 0, 1 left, 2, 3 right
    order2 = [0, 2, 1, 3]                                     # keyframe 2: left features first
    k2 = [px(T2, r2[i], pts[i]) for i in order2]
    m = np.empty(4, np.int32)
    m[order2] = np.arange(4)
    kf1 = _keyframe(tc._keys(k1, np.zeros(4, int), np.zeros(4)), 1, cam, cam2, True, 2)
    kf2 = _keyframe(tc._keys(k2, np.zeros(4, int), np.zeros(4)), 1, cam, cam2, True, 2)
    return dict(name="four_pairings", kf1=kf1, g1=geometry(T1, cam, Trl), kf2=kf2, g2=geometry(T2, cam, Trl), matches12=m.reshape(1, 4),
                params=dict(inertial=False, far_points=False, th_far=0.0, ratio_factor=RATIO_FACTOR), status=np.ones(4, np.int32),
                pairings=pairing, truth=pts)


def directed():
    return hand_built() + [four_pairings()]


def to_device_geometry(orb, g):
    return orb.NewPointGeometry(g["Tcw"], g["Ow"], [g["fx"], g["fy"], g["cx"], g["cy"]], g["mb"], g["mbf"], g["Tcw_right"], g["Ow_right"],
                                g["Rwc"], g["twc"], g["depth"], g["keys_raw"], g["invfx"], g["invfy"], g["kb8_precision"])

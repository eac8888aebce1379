"""ORBmatcher::SearchForTriangulation restated in Python, statement by statement, in the reference's SEQUENTIAL form (reference
src/ORBmatcher.cc:1006-1245): the lower_bound walk over the two FeatureVectors, the scan that skips on `dist > bestDist` in front
of the epipole test and the constraint, the rotation histogram, ComputeThreeMaxima and the removal.

The checker of ft_search_for_triangulation.  What it does not state itself is taken from the oracle, where existing tests pin
it: ComputeThreeMaxima (orc_three_maxima), KannalaBrandt8::TriangulateMatches (oracle.binding.kb8_triangulate, with a rig made
of the two cameras and the pose of the pairing: KannalaBrandt8::epipolarConstrain is TriangulateMatches(...) > 0.0001f,
src/CameraModels/KannalaBrandt8.cpp:216-220); DescriptorDistance is the popcount of the XOR and the rotation bin the one of
init_search_ref.  Pinhole::epipolarConstrain (src/CameraModels/Pinhole.cpp:107-129) is written out behind the F12 it is given.
All arithmetic is float32 with every operation rounded on its own (numpy scalars: no fused operations).  The constants of a
pair (ep, F12, R12, t12) are inputs, as for the library.  Besides the function's outputs it reports what happened on the way,
so that a test can assert that its inputs exercise the order-dependent parts at all.

A keyframe is a dict: keys (KP_DTYPE records: mvKeysUn, or mvKeys then mvKeysRight), descriptors, fv_nodes / fv_offsets /
fv_features (mFeatVec, CSR), has_point, uright (or None = all -1), n_left, two_cameras, cam_model (0 pinhole, 1 KannalaBrandt8),
cam, cam2, scale_factors, level_sigma2.  A pair is a dict: ep, F12 (3 x 3), R12 (4 x 3 x 3: T12 or ll, then lr, rl, rr), t12
(4 x 3), kb8_precision.
"""
import numpy as np

from oracle import binding as ob
from tests.init_search_ref import HISTO_LENGTH, TH_LOW, distances, rotation_bin, three_maxima

f32 = np.float32


def pinhole_constrain(F12, kp1, kp2, unc):
    """Pinhole::epipolarConstrain behind F12 (:114-128): a*x means f32(a * x), sums left to right"""
    F = np.asarray(F12, f32).reshape(3, 3)
    x1, y1, x2, y2 = f32(kp1["x"]), f32(kp1["y"]), f32(kp2["x"]), f32(kp2["y"])
    a = f32(f32(f32(x1 * F[0, 0]) + f32(y1 * F[1, 0])) + F[2, 0])
    b = f32(f32(f32(x1 * F[0, 1]) + f32(y1 * F[1, 1])) + F[2, 1])
    c = f32(f32(f32(x1 * F[0, 2]) + f32(y1 * F[1, 2])) + F[2, 2])
    num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
    den = f32(f32(a * a) + f32(b * b))
    if den == 0:
        return False
    with np.errstate(all="ignore"):
        dsqr = f32(f32(num * num) / den)
    return bool(float(dsqr) < 3.84 * float(f32(unc)))


def kb8_constrain(cam_a, cam_b, R12, t12, precision, kp1, kp2, sigma1, sigma2, calls=None):
    """KannalaBrandt8::epipolarConstrain: this = cam_a, pCamera2 = cam_b"""
    if calls is not None:
        calls.append((tuple(f32(v) for v in cam_a), tuple(f32(v) for v in cam_b), np.asarray(R12, f32).copy(), np.asarray(t12, f32).copy()))
    rig = ob.make_rig(cam_a, cam_b, R12, t12, precision)
    code, _ = ob.kb8_triangulate(rig, [[kp1["x"], kp1["y"]]], [[kp2["x"], kp2["y"]]], [sigma1], [sigma2])
    return bool(code[0] > f32(0.0001))


def _lower_bound(nodes, it, key):
    """std::map::lower_bound from the front of the sorted keys (the walk only ever moves forward)"""
    return int(np.searchsorted(nodes, key, side="left"))


def search_for_triangulation(kf1, kf2, pair, only_stereo=False, coarse=False, check_orientation=True, calls=None):
    """-> dict(matches12, n, best_dist, pairs, stats)"""
    N1 = len(kf1["keys"])
    keys1, keys2 = kf1["keys"], kf2["keys"]
    two1, two2 = bool(kf1["two_cameras"]), bool(kf2["two_cameras"])
    ep = np.asarray(pair["ep"], f32).reshape(2)
    R = np.asarray(pair["R12"], f32).reshape(-1, 3, 3)
    t = np.asarray(pair["t12"], f32).reshape(-1, 3)
    cam1, cam2 = kf1["cam"], kf2["cam"]                      # pCamera1, pCamera2 (:1025)
    R12, t12 = R[0], t[0]                                    # T12 (:1028-1030); two cameras choose per candidate
    nmatches = 0
    m12 = np.full(N1, -1, np.int32)
    best_dist = np.full(N1, TH_LOW, np.int32)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    st = dict(shared_nodes=0, scanned=0, constraint_calls=0, constraint_rejections=0, nearest_rejected=0, next_won=0,
              epipole_rejections=0, ties=0, removed_by_histogram=0, node_sizes=set())
    nodes1, nodes2 = np.asarray(kf1["fv_nodes"]), np.asarray(kf2["fv_nodes"])
    off1, off2 = kf1["fv_offsets"], kf2["fv_offsets"]
    i1, i2 = 0, 0
    while i1 < len(nodes1) and i2 < len(nodes2):
        if nodes1[i1] == nodes2[i2]:
            st["shared_nodes"] += 1
            list1 = kf1["fv_features"][off1[i1]:off1[i1 + 1]]
            list2 = kf2["fv_features"][off2[i2]:off2[i2 + 1]]
            st["node_sizes"].add(len(list2))
            for idx1 in [int(v) for v in list1]:
                if kf1["has_point"][idx1]:                   # pMP1 (:1073)
                    continue
                stereo1 = (not two1) and kf1["uright"] is not None and kf1["uright"][idx1] >= 0
                if only_stereo and not stereo1:
                    continue
                kp1 = keys1[idx1]
                right1 = not (kf1["n_left"] == -1 or idx1 < kf1["n_left"])
                dists = distances(kf1["descriptors"][idx1], kf2["descriptors"][list2]) if len(list2) else []
                bd, bi = TH_LOW, -1
                nearest_reaching = None
                for idx2, dist in zip([int(v) for v in list2], [int(v) for v in dists]):
                    if kf2["has_point"][idx2]:               # vbMatched2 is never written (:1048)
                        continue
                    stereo2 = (not two2) and kf2["uright"] is not None and kf2["uright"][idx2] >= 0
                    if only_stereo and not stereo2:
                        continue
                    st["scanned"] += 1
                    if dist > TH_LOW or dist > bd:           # :1116
                        continue
                    kp2 = keys2[idx2]
                    right2 = not (kf2["n_left"] == -1 or idx2 < kf2["n_left"])
                    if not stereo1 and not stereo2 and not two1:
                        distex = f32(ep[0] - f32(kp2["x"]))
                        distey = f32(ep[1] - f32(kp2["y"]))
                        if f32(f32(distex * distex) + f32(distey * distey)) < f32(f32(100) * f32(kf2["scale_factors"][kp2["octave"]])):
                            st["epipole_rejections"] += 1
                            continue
                    if two1 and two2:                        # :1135-1169
                        k = (2 if right1 else 0) + (1 if right2 else 0)
                        R12, t12 = R[k], t[k]
                        cam1 = kf1["cam2"] if right1 else kf1["cam"]
                        cam2 = kf2["cam2"] if right2 else kf2["cam"]
                    nearest_reaching = dist if nearest_reaching is None else min(nearest_reaching, dist)
                    ok = bool(coarse)
                    if not ok:
                        st["constraint_calls"] += 1
                        s1 = kf1["level_sigma2"][kp1["octave"]]
                        s2 = kf2["level_sigma2"][kp2["octave"]]
                        if kf1["cam_model"] == 0:
                            ok = pinhole_constrain(pair["F12"], kp1, kp2, s2)
                        else:
                            ok = kb8_constrain(cam1, cam2, R12, t12, pair.get("kb8_precision", 1e-6), kp1, kp2, s1, s2, calls)
                        st["constraint_rejections"] += int(not ok)
                    if ok:
                        st["ties"] += int(bi >= 0 and dist == bd)
                        bi, bd = idx2, dist
                best_dist[idx1] = bd
                if nearest_reaching is not None and (bi < 0 or bd > nearest_reaching):
                    st["nearest_rejected"] += 1
                    st["next_won"] += int(bi >= 0)
                if bi >= 0:
                    m12[idx1] = bi
                    nmatches += 1
                    if check_orientation:
                        b = rotation_bin(kp1["angle"], keys2[bi]["angle"])
                        assert 0 <= b < HISTO_LENGTH
                        rot_hist[b].append(idx1)
            i1 += 1
            i2 += 1
        elif nodes1[i1] < nodes2[i2]:
            i1 = _lower_bound(nodes1, i1, nodes2[i2])
        else:
            i2 = _lower_bound(nodes2, i2, nodes1[i1])
    if check_orientation:
        keep = three_maxima([len(b) for b in rot_hist])
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for idx1 in rot_hist[b]:
                m12[idx1] = -1
                nmatches -= 1
                st["removed_by_histogram"] += 1
    pairs = [(i, int(m12[i])) for i in range(N1) if m12[i] >= 0]
    return dict(matches12=m12, n=nmatches, best_dist=best_dist, pairs=pairs, stats=st)

"""ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist) restated in Python, statement
by statement (reference src/ORBmatcher.cc:2087-2208).

The checker of ft_search_keyframe_projection / ft_tracked_frame_search_keyframe_projection.  What it does not state itself is
taken from the oracle, where existing tests pin it: the candidates of a window and their order (oracle.binding.features_in_area
= Frame::GetFeaturesInArea), ComputeThreeMaxima (orc_three_maxima) and Sophus::SE3f * point (oracle.binding.SE3.apply; also
for Ow = Tcw.inverse().translation(): the conjugate quaternion with zero translation applied to -t); rotation_bin and
distances are init_search_ref's.  All arithmetic is float32 with every operation rounded on its own (numpy scalars: no fused
operations); logf, ceilf, sqrtf, atan2f, cosf, sinf are the host's glibc, which the oracle links.  The projection follows
projectCam of oracle/orb_oracle.cpp:1108-1125 for both camera models.  test_reloc_search_cpu.py pins the restatement against
the oracle's last-frame search and isInFrustum.  Besides the function's outputs it reports what happened on the way, so that a
test can assert that its inputs exercise the sequential part at all.
"""
import ctypes as C

import numpy as np

from oracle import binding as ob
from tests.init_search_ref import HISTO_LENGTH, distances, rotation_bin, three_maxima

f32 = np.float32
_libm = C.CDLL("libm.so.6")
for _n, _k in (("logf", 1), ("ceilf", 1), ("sqrtf", 1), ("cosf", 1), ("sinf", 1), ("atan2f", 2)):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float] * _k


def _m(name, *a):
    return f32(getattr(_libm, name)(*[float(v) for v in a]))


def project(cam_model, cam, p):
    """mpCamera->project(x3Dc): Pinhole.cpp:43-49 / KannalaBrandt8.cpp:67-84 as projectCam of the oracle states them"""
    cam = [f32(c) for c in cam]
    x, y, z = [f32(v) for v in p]
    with np.errstate(all="ignore"):
        if cam_model == 0:
            return f32(f32(f32(cam[0] * x) / z) + cam[2]), f32(f32(f32(cam[1] * y) / z) + cam[3])
        x2y2 = f32(f32(x * x) + f32(y * y))
        theta = _m("atan2f", _m("sqrtf", x2y2), z)
        psi = _m("atan2f", y, x)
        t2 = f32(theta * theta)
        t3 = f32(theta * t2)
        t5 = f32(t3 * t2)
        t7 = f32(t5 * t2)
        t9 = f32(t7 * t2)
        r = f32(f32(f32(f32(theta + f32(cam[4] * t3)) + f32(cam[5] * t5)) + f32(cam[6] * t7)) + f32(cam[7] * t9))
        return (f32(f32(f32(cam[0] * r) * _m("cosf", psi)) + cam[2]), f32(f32(f32(cam[1] * r) * _m("sinf", psi)) + cam[3]))


def camera_centre(Tcw: "ob.SE3"):
    """Ow = Tcw.inverse().translation() (:2092): so3().inverse() * (translation() * -1)"""
    q = Tcw.q
    conj = ob.SE3(np.array([-q[0], -q[1], -q[2], q[3]], f32), np.zeros(3, f32))
    return conj.apply((-Tcw.t).astype(f32))


def predict_scale(max_distance_raw, dist, log_scale_factor, nlevels):
    """MapPoint::PredictScale(dist, Frame*) (src/MapPoint.cc:531-546)"""
    ratio = f32(f32(max_distance_raw) / f32(dist))
    n = int(_m("ceilf", f32(_m("logf", ratio) / f32(log_scale_factor))))
    return 0 if n < 0 else (nlevels - 1 if n >= nlevels else n)


def search_by_projection(F: "ob.FrameView", kf: dict, Tcw: "ob.SE3", log_scale_factor, th, orb_dist, check_orientation=True):
    """F: an oracle FrameView (its holder_obs is the state on entry: held <=> != -1; NOT modified); kf: dict(valid, world_pos,
    max_distance, min_distance, descriptors, observations, angle) over pKF->GetMapPointMatches().
    -> dict(assign, n, holder_obs, best_dist, best_idx, level, searched, zc, Ow, stats)."""
    N = len(kf["valid"])
    nleft = F.N if F.Nleft == -1 else F.Nleft
    keys2, desc2 = F.keys, F.descriptors
    cam = [F.c.cam[i] for i in range(8)]
    minx, miny, maxx, maxy = f32(F.c.mnMinX), f32(F.c.mnMinY), f32(F.c.mnMaxX), f32(F.c.mnMaxY)
    holder = F.holder_obs.copy()
    before = holder != -1
    occupied = before.copy()                      # CurrentFrame.mvpMapPoints[i2] != NULL
    assign = np.full(F.N, -1, np.int32)
    best_dist, best_idx = np.full(N, 256, np.int32), np.full(N, -1, np.int32)
    level_of, searched, zc = np.full(N, -1, np.int32), np.zeros(N, bool), np.zeros(N, f32)
    Ow = camera_centre(Tcw)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    st = dict(projected=0, searched=0, locked_skips=0, locked_before=0, changed_by_locks=0, accepted=0, removed_by_histogram=0,
              levels=set())
    for i in range(N):
        if not kf["valid"][i]:                     # pMP && !pMP->isBad() && !sAlreadyFound.count(pMP)
            continue
        xw = np.asarray(kf["world_pos"][i], f32)
        xc = Tcw.apply(xw)
        zc[i] = xc[2]
        u, v = project(F.c.cam_model, cam, xc)
        if u < minx or u > maxx:
            continue
        if v < miny or v > maxy:
            continue
        st["projected"] += 1
        po = (xw - Ow).astype(f32)
        sq = [f32(po[k] * po[k]) for k in range(3)]
        dist3d = _m("sqrtf", f32(sq[0] + f32(sq[1] + sq[2])))     # Eigen's norm(): e0 + (e1 + e2)
        max_d = f32(f32(1.2) * f32(kf["max_distance"][i]))        # GetMaxDistanceInvariance()
        min_d = f32(f32(0.8) * f32(kf["min_distance"][i]))
        if dist3d < min_d or dist3d > max_d:
            continue
        level = predict_scale(kf["max_distance"][i], dist3d, log_scale_factor, len(F.sf))
        level_of[i], searched[i] = level, True
        st["searched"] += 1
        st["levels"].add(level)
        radius = f32(f32(th) * F.sf[level])
        idx2 = ob.features_in_area(F, float(u), float(v), float(radius), level - 1, level + 1)
        if len(idx2) == 0:
            continue
        assert idx2.max() < nleft                  # bRight defaults to false: left keypoints only
        dists = distances(kf["descriptors"][i], desc2[idx2])
        bd, bi = 256, -1
        free_d, free_i = 256, -1                   # the same loop without the lock test (for the statistics only)
        for i2, dist in zip(idx2.tolist(), dists.tolist()):
            if dist < free_d:
                free_d, free_i = dist, i2
            if occupied[i2]:
                st["locked_skips"] += 1
                st["locked_before"] += int(before[i2])
                continue
            if dist < bd:
                bd, bi = dist, i2
        best_dist[i], best_idx[i] = bd, bi
        if free_d <= orb_dist and free_i != (bi if bd <= orb_dist else -1):
            st["changed_by_locks"] += 1
        if bd <= orb_dist:
            occupied[bi] = True
            assign[bi] = i
            holder[bi] = kf["observations"][i]
            nmatches += 1
            st["accepted"] += 1
            if check_orientation:
                b = rotation_bin(kf["angle"][i], keys2["angle"][bi])
                assert 0 <= b < HISTO_LENGTH
                rot_hist[b].append(bi)
    if check_orientation:
        keep = three_maxima([len(b) for b in rot_hist])
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for i2 in rot_hist[b]:
                assign[i2] = -1
                holder[i2] = -1
                nmatches -= 1
                st["removed_by_histogram"] += 1
    return dict(assign=assign, n=nmatches, holder_obs=holder, best_dist=best_dist, best_idx=best_idx, level=level_of,
                searched=searched, zc=zc, Ow=Ow, stats=st)

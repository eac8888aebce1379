"""ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) (reference src/ORBmatcher.cc:1247-1437) and ORBmatcher::Fuse(pKF, Scw, vpPoints, th,
vpReplacePoint) (:1439-1554) restated in Python, statement by statement, without the map bookkeeping behind the candidate loop
(:1411-1430, :1536-1550) - `fuse` - and with it on Python objects - `fuse_inline`, `apply_in_order`.

The checker of ft_fuse_search.  What it does not state itself is taken where existing tests pin it: the candidates of a window and
their order (oracle.binding.features_in_area = KeyFrame::GetFeaturesInArea, whose cells, cell order and box are those of
Frame::GetFeaturesInArea - src/KeyFrame.cc:704-748 against src/Frame.cc:681-747 - called without a level filter), Sophus::SE3f *
point (oracle.binding.SE3.apply), the camera models, MapPoint::PredictScale and Tcw.inverse().translation() (reloc_search_ref's
project, predict_scale, camera_centre).  All arithmetic is float32 with every operation rounded on its own (numpy scalars: no
fused operations); logf, ceilf, sqrtf, atan2f, cosf, sinf are the host's glibc.  The two comparisons the reference makes in
double - `PO.dot(Pn)<0.5*dist3D` and `e2*mvInvLevelSigma2[kpLevel]>7.8` / `>5.99` - are made in double here.
test_fuse_cpu.py pins projection, distance range, viewing angle and level against the oracle's isInFrustum.  Besides the outputs
it reports what happened on the way, so that a test can assert that its inputs exercise every exit and the chi-square test."""
import numpy as np

from oracle import binding as ob
from tests.init_search_ref import distances
from tests.reloc_search_ref import _m, camera_centre, f32, predict_scale, project

TH_LOW = 50
SEARCHED, SKIPPED, DEPTH, IMAGE, DISTANCE, NORMAL, EMPTY = range(7)


def inv_level_sigma2(sf):
    """mvInvLevelSigma2 as ORBextractor builds it (src/ORBextractor.cc:432-440): 1.0f / (mvScaleFactor[i] * mvScaleFactor[i])"""
    return np.array([f32(1.0) / f32(f32(s) * f32(s)) for s in sf], np.float32)


def front(F, cam, Tcw, Ow, log_sf, th, xw, pn, max_raw, min_raw):
    """:1297-1343 of one point -> (stage, u, v, ur, level, radius, dist3D, dot, zc)"""
    xw = np.asarray(xw, f32)
    xc = Tcw.apply(xw)
    if xc[2] < f32(0.0):
        return DEPTH, None, None, None, -1, None, None, None, xc[2]
    with np.errstate(all="ignore"):
        invz = f32(f32(1.0) / xc[2])
        u, v = project(F.c.cam_model, cam, xc)
        if not (u >= f32(F.c.mnMinX) and u < f32(F.c.mnMaxX) and v >= f32(F.c.mnMinY) and v < f32(F.c.mnMaxY)):   # KeyFrame::IsInImage
            return IMAGE, u, v, None, -1, None, None, None, xc[2]
        ur = f32(u - f32(f32(F.c.mbf) * invz))
    po = [f32(xw[k] - f32(Ow[k])) for k in range(3)]
    sq = [f32(po[k] * po[k]) for k in range(3)]
    dist3d = _m("sqrtf", f32(sq[0] + f32(sq[1] + sq[2])))            # Eigen's norm(): e0 + (e1 + e2)
    max_d, min_d = f32(f32(1.2) * f32(max_raw)), f32(f32(0.8) * f32(min_raw))
    if dist3d < min_d or dist3d > max_d:
        return DISTANCE, u, v, ur, -1, None, dist3d, None, xc[2]
    pr = [f32(po[k] * f32(pn[k])) for k in range(3)]
    dot = f32(pr[0] + f32(pr[1] + pr[2]))                            # Eigen's dot(): the same association
    if float(dot) < 0.5 * float(dist3d):
        return NORMAL, u, v, ur, -1, None, dist3d, dot, xc[2]
    level = predict_scale(max_raw, dist3d, log_sf, len(F.sf))
    return SEARCHED, u, v, ur, level, f32(f32(th) * F.sf[level]), dist3d, dot, xc[2]


def candidates(F, right, check_reprojection, inv_sigma2, pt, desc):
    """:1345-1408 of a point that reached the window, pt = front(...) -> (stage, bestDist, bestIdx, statistics of the point)"""
    _, u, v, ur, level, radius = pt[:6]
    st = dict(window=0, band=0, chi_stereo=0, chi_mono=0, tie=False, free=(256, -1))
    idx = ob.features_in_area(F, float(u), float(v), float(radius), -1, -1, right)
    st["window"] = len(idx)
    if len(idx) == 0:
        return EMPTY, 256, -1, st
    nleft = 0 if F.Nleft == -1 else F.Nleft
    keys = F.keys_right if right else F.keys
    rows = idx + nleft if right else idx
    dists = distances(desc, F.descriptors[rows])
    bd, bi = 256, -1
    fd, fi = 256, -1                               # the same loop without the chi-square test (for the statistics only)
    for i2, row, dist in zip(idx.tolist(), rows.tolist(), dists.tolist()):
        kp = keys[i2]
        oct_ = int(kp["octave"])
        if oct_ < level - 1 or oct_ > level:
            continue
        st["band"] += 1
        if dist < fd:
            fd, fi = dist, row
        elif dist == fd:
            st["tie"] = True
        if check_reprojection:
            ex, ey = f32(u - f32(kp["x"])), f32(v - f32(kp["y"]))
            uright = F.uright[i2] if (F.uright is not None and F.Nleft == -1) else f32(-1.0)   # pKF->mvuRight[idx] (idx before += NLeft)
            if uright >= 0:
                er = f32(ur - f32(uright))
                e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))
                if float(f32(e2 * inv_sigma2[oct_])) > 7.8:
                    st["chi_stereo"] += 1
                    continue
            else:
                e2 = f32(f32(ex * ex) + f32(ey * ey))
                if float(f32(e2 * inv_sigma2[oct_])) > 5.99:
                    st["chi_mono"] += 1
                    continue
        if dist < bd:
            bd, bi = dist, row
    st["free"] = (fd, fi)
    return SEARCHED, bd, bi, st


def fuse(F, points, Tcw, Ow, log_sf, th, right=False, cam2=None, valid=None, check_reprojection=True, inv_sigma2=None):
    """F: an oracle FrameView of the keyframe; points: dict(world_pos, normal, max_distance, min_distance, descriptors);
    check_reprojection False: the Sim3 overload.  -> dict(best_idx, best_dist, stage, n_found, level, u, v, dot, dist, zc, stats)"""
    M = len(points["world_pos"])
    cam = [F.c.cam[i] for i in range(8)] if not right else [float(c) for c in cam2]
    inv_sigma2 = inv_level_sigma2(F.sf) if inv_sigma2 is None else np.asarray(inv_sigma2, np.float32)
    best_idx, best_dist, stage = np.full(M, -1, np.int32), np.full(M, 256, np.int32), np.zeros(M, np.uint8)
    level = np.full(M, -1, np.int32)
    u, v, dot, dist, zc = [np.full(M, np.nan, np.float32) for _ in range(5)]
    st = dict(stages=[0] * 7, chi_stereo=0, chi_mono=0, changed_by_chi=0, fused_changed_by_chi=0, ties=0, max_window=0, levels=set())
    for i in range(M):
        if valid is not None and not valid[i]:
            stage[i] = SKIPPED
            st["stages"][SKIPPED] += 1
            continue
        pt = front(F, cam, Tcw, Ow, log_sf, th, points["world_pos"][i], points["normal"][i], points["max_distance"][i], points["min_distance"][i])
        zc[i] = pt[8]
        for a, k in ((u, 1), (v, 2), (dist, 6), (dot, 7)):
            if pt[k] is not None:
                a[i] = pt[k]
        s = pt[0]
        if s == SEARCHED:
            level[i] = pt[4]
            st["levels"].add(pt[4])
            s, bd, bi, ps = candidates(F, right, check_reprojection, inv_sigma2, pt, points["descriptors"][i])
            best_dist[i], best_idx[i] = bd, bi
            st["chi_stereo"] += ps["chi_stereo"]
            st["chi_mono"] += ps["chi_mono"]
            st["ties"] += int(ps["tie"])
            st["max_window"] = max(st["max_window"], ps["window"])
            fd, fi = ps["free"]
            if (fd, fi) != (bd, bi):               # bestDist / bestIdx as the loop leaves them, with and without the test
                st["changed_by_chi"] += 1
                st["fused_changed_by_chi"] += int((fi if fd <= TH_LOW else -1) != (bi if bd <= TH_LOW else -1))
        stage[i] = s
        st["stages"][s] += 1
    return dict(best_idx=best_idx, best_dist=best_dist, stage=stage, n_found=int((best_dist <= TH_LOW).sum()), level=level, u=u, v=v,
                dot=dot, dist=dist, zc=zc, stats=st)


# ---- the bookkeeping behind the loop, on Python objects (what stays with the caller of ft_fuse_search) ----
class MP:
    """the fields of a MapPoint that Fuse's bookkeeping reads and writes"""

    def __init__(self, i, observations):
        self.i, self.bad, self.obs, self.in_kf, self.replaced = i, False, observations, False, None


def bookkeeping(pMP, slots, best_idx):
    """:1413-1428 for a point whose bestDist <= TH_LOW; slots[idx] = pKF->GetMapPoint(idx)"""
    other = slots.get(best_idx)
    if other is not None:
        if not other.bad:
            if other.obs > pMP.obs:                # pMP->Replace(pMPinKF): pMP goes bad
                pMP.bad, pMP.replaced = True, other
            else:                                  # pMPinKF->Replace(pMP): pMP takes the slot
                other.bad, other.replaced = True, pMP
                other.in_kf = False
                slots[best_idx] = pMP
                pMP.in_kf = True
                pMP.obs += other.obs
    else:
        slots[best_idx] = pMP                      # AddObservation, AddMapPoint
        pMP.in_kf = True
        pMP.obs += 1


def fuse_inline(F, points, vp, slots, Tcw, Ow, log_sf, th):
    """Fuse(pKF, vpMapPoints, th) as the reference runs it: test 1 at the top of every iteration, the bookkeeping inside the loop.
    vp[i] = the MP object of list entry i (one object may be listed more than once) or None -> nFused"""
    cam = [F.c.cam[i] for i in range(8)]
    inv_sigma2 = inv_level_sigma2(F.sf)
    n = 0
    for i, pMP in enumerate(vp):
        if pMP is None or pMP.bad or pMP.in_kf:
            continue
        pt = front(F, cam, Tcw, Ow, log_sf, th, points["world_pos"][i], points["normal"][i], points["max_distance"][i], points["min_distance"][i])
        if pt[0] != SEARCHED:
            continue
        s, bd, bi, _ = candidates(F, False, True, inv_sigma2, pt, points["descriptors"][i])
        if s == SEARCHED and bd <= TH_LOW:
            bookkeeping(pMP, slots, bi)
            n += 1
    return n


def apply_in_order(res, vp, slots):
    """the caller's loop behind a one-target ft_fuse_search: in index order, test 1 again, then the bookkeeping -> nFused"""
    n = 0
    for i, pMP in enumerate(vp):
        if pMP is None or pMP.bad or pMP.in_kf:    # (what `valid` said at call time may have turned since)
            continue
        if res["best_dist"][i] <= TH_LOW:
            bookkeeping(pMP, slots, int(res["best_idx"][i]))
            n += 1
    return n

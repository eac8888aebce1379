"""ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (reference src/ORBmatcher.cc:526-631) and its
overload with vpPointsKFs / vpMatchedKF (:633-745) restated in Python, twice:

`search`            the literal loop, statement by statement.  The tests in front of the window are fuse_ref.front (the Sim3 overload
                    of Fuse, :1461-1503, pinned against the oracle's isInFrustum by test_fuse_cpu.py) for the overload that calls
                    mpCamera->project (:564); `front_hand` is the same text with the projection of :672-677 written out.  The window
                    is oracle.binding.features_in_area (KeyFrame::GetFeaturesInArea of the left camera, no level filter), in its order.
`search_compacted`  the formulation the library runs: per point the candidates that are free on entry, lie in the band and are no
                    farther than the integer threshold, as (distance, position in GetFeaturesInArea's order); then a walk over the
                    points that have candidates, in index order, each taking its smallest candidate not taken before.

All arithmetic is float32 with every operation rounded on its own (numpy scalars).  vpMatched is an int32 array: -1 = NULL, anything
else = held; a point that writes stores its own index.  Both return dict(matched, point_keypoint, stage, n_matches, stats)."""
import numpy as np

from oracle import binding as ob
from tests import fuse_ref as fref
from tests.init_search_ref import distances
from tests.reloc_search_ref import _m, f32, predict_scale

TH_LOW = 50
WROTE, SKIPPED, DEPTH, IMAGE, DISTANCE, NORMAL, EMPTY, NOWRITE = range(8)
TOP = 4   # the library's top record (statistics only)


def threshold(ratio):
    """the largest d of 0 .. 255 with (float)d <= (float)50 * ratio, None where the reference would write vpMatched[-1]"""
    prod = f32(f32(TH_LOW) * f32(ratio))
    if not (prod >= 0 and prod < 256):
        return None
    return max(d for d in range(256) if f32(d) <= prod)


def front_hand(F, cam, Tcw, Ow, log_sf, th, xw, pn, max_raw, min_raw):
    """:654-701 of one point: fuse_ref.front with the projection written out by hand -> (stage, u, v, None, level, radius, ...)"""
    xw = np.asarray(xw, f32)
    xc = Tcw.apply(xw)
    if xc[2] < f32(0.0):
        return fref.DEPTH, None, None, None, -1, None, None, None, xc[2]
    with np.errstate(all="ignore"):
        invz = f32(f32(1.0) / xc[2])
        x, y = f32(xc[0] * invz), f32(xc[1] * invz)
        u, v = f32(f32(f32(cam[0]) * x) + f32(cam[2])), f32(f32(f32(cam[1]) * y) + f32(cam[3]))    # pKF->fx, fy, cx, cy
        if not (u >= f32(F.c.mnMinX) and u < f32(F.c.mnMaxX) and v >= f32(F.c.mnMinY) and v < f32(F.c.mnMaxY)):   # KeyFrame::IsInImage
            return fref.IMAGE, u, v, None, -1, None, None, None, xc[2]
    po = [f32(xw[k] - f32(Ow[k])) for k in range(3)]
    sq = [f32(po[k] * po[k]) for k in range(3)]
    dist3d = _m("sqrtf", f32(sq[0] + f32(sq[1] + sq[2])))
    max_d, min_d = f32(f32(1.2) * f32(max_raw)), f32(f32(0.8) * f32(min_raw))
    if dist3d < min_d or dist3d > max_d:
        return fref.DISTANCE, u, v, None, -1, None, dist3d, None, xc[2]
    pr = [f32(po[k] * f32(pn[k])) for k in range(3)]
    dot = f32(pr[0] + f32(pr[1] + pr[2]))
    if float(dot) < 0.5 * float(dist3d):
        return fref.NORMAL, u, v, None, -1, None, dist3d, dot, xc[2]
    level = predict_scale(max_raw, dist3d, log_sf, len(F.sf))
    return fref.SEARCHED, u, v, None, level, f32(f32(th) * F.sf[level]), dist3d, dot, xc[2]


def _front(F, cam, Tcw, Ow, log_sf, th, points, i, hand_pinhole):
    fn = front_hand if hand_pinhole else fref.front
    return fn(F, cam, Tcw, Ow, log_sf, int(th), points["world_pos"][i], points["normal"][i], points["max_distance"][i], points["min_distance"][i])


def _outputs(F, M, matched):
    matched = np.array(matched, np.int32, copy=True)
    assert matched.shape == (F.c.N,)
    return matched, np.full(M, -1, np.int32), np.zeros(M, np.uint8)


def search(F, points, Tcw, Ow, log_sf, th, ratio, matched, valid=None, hand_pinhole=False):
    """the literal loop.  F: an oracle FrameView of the keyframe; matched: vpMatched on entry (not modified)"""
    M = len(points["world_pos"])
    cam = [F.c.cam[i] for i in range(8)]
    entry = np.array(matched, np.int32, copy=True)
    matched, pk, stage = _outputs(F, M, matched)
    prod = f32(f32(TH_LOW) * f32(ratio))                      # `TH_LOW*ratioHamming`: int * float
    assert threshold(ratio) is not None
    st = dict(stages=[0] * 8, held_on_entry=0, changed_by_locks=0, levels=set(), max_candidates=0, walk=0, ties=0)
    n = 0
    for i in range(M):
        if valid is not None and not valid[i]:               # isBad() || spAlreadyFound.count(pMP)
            stage[i] = SKIPPED
            continue
        pt = _front(F, cam, Tcw, Ow, log_sf, th, points, i, hand_pinhole)
        if pt[0] != fref.SEARCHED:
            stage[i] = pt[0]
            continue
        u, v, level, radius = pt[1], pt[2], pt[4], pt[5]
        st["levels"].add(level)
        idx = ob.features_in_area(F, float(u), float(v), float(radius), -1, -1, False)
        if len(idx) == 0:
            stage[i] = EMPTY
            continue
        dists = distances(points["descriptors"][i], F.descriptors[idx])
        bd, bi = 256, -1
        bd0, bi0, ncand = 256, -1, 0                          # the same loop against vpMatched as on entry (statistics only)
        for i2, dist in zip(idx.tolist(), dists.tolist()):
            oct_ = int(F.keys[i2]["octave"])
            in_band = not (oct_ < level - 1 or oct_ > level)
            if entry[i2] != -1:
                st["held_on_entry"] += int(in_band)
            elif in_band:
                ncand += int(f32(dist) <= prod)
                if dist < bd0:
                    bd0, bi0 = dist, i2
                elif dist == bd0:
                    st["ties"] += 1
            if matched[i2] != -1:                             # `if(vpMatched[idx]) continue;`
                continue
            if not in_band:
                continue
            if dist < bd:
                bd, bi = dist, i2
        st["max_candidates"] = max(st["max_candidates"], ncand)
        st["walk"] += int(ncand > 0)
        wrote = -1
        if f32(bd) <= prod:                                   # `bestDist<=TH_LOW*ratioHamming`
            matched[bi] = i
            wrote = bi
            n += 1
        pk[i] = wrote
        stage[i] = WROTE if wrote >= 0 else NOWRITE
        st["changed_by_locks"] += int(wrote != (bi0 if f32(bd0) <= prod else -1))
    for s in stage.tolist():
        st["stages"][s] += 1
    return dict(matched=matched, point_keypoint=pk, stage=stage, n_matches=n, stats=st)


def search_compacted(F, points, Tcw, Ow, log_sf, th, ratio, matched, valid=None, hand_pinhole=False):
    """candidates within the threshold first, then the walk over the points that have some"""
    M = len(points["world_pos"])
    cam = [F.c.cam[i] for i in range(8)]
    matched, pk, stage = _outputs(F, M, matched)
    thr = threshold(ratio)
    cands, walk = {}, []
    for i in range(M):
        if valid is not None and not valid[i]:
            stage[i] = SKIPPED
            continue
        pt = _front(F, cam, Tcw, Ow, log_sf, th, points, i, hand_pinhole)
        if pt[0] != fref.SEARCHED:
            stage[i] = pt[0]
            continue
        u, v, level, radius = pt[1], pt[2], pt[4], pt[5]
        idx = ob.features_in_area(F, float(u), float(v), float(radius), -1, -1, False)
        if len(idx) == 0:
            stage[i] = EMPTY
            continue
        stage[i] = NOWRITE
        dists = distances(points["descriptors"][i], F.descriptors[idx])
        keys = [(dist, rank, i2) for rank, (i2, dist) in enumerate(zip(idx.tolist(), dists.tolist()))
                if matched[i2] == -1 and level - 1 <= int(F.keys[i2]["octave"]) <= level and dist <= thr]
        if keys:
            cands[i] = sorted(keys)
            walk.append(i)
    taken, n, past_top = set(), 0, 0
    for i in walk:
        free = [k for k in cands[i] if k[2] not in taken]
        if not free:
            continue
        past_top += int(all(k[2] in taken for k in cands[i][:TOP]))
        i2 = free[0][2]
        taken.add(i2)
        matched[i2] = i
        pk[i] = i2
        stage[i] = WROTE
        n += 1
    return dict(matched=matched, point_keypoint=pk, stage=stage, n_matches=n, stats=dict(walk=len(walk), past_top=past_top))

"""Seeded synthetic scenarios shared by the oracle tests (CPU) and the parity tests (GPU)."""
import numpy as np

from fasttrack_amd import synth
from fasttrack_amd.scenarios import (GEOMETRY_BOUNDS, KB8_CAM, LATTICE_SHIFTED_BOUNDS, bow_match_scenario, fisheye_rig_scenario, frame_bounds, grid_cells,  # noqa: F401
                                     kb8_project64, last_frame_scenario, lattice_last_frame, local_points_from_frustum,
                                     local_points_scenario, map_points_scenario, random_pose, random_se3)
from oracle import binding as ob

KP = ob.KP_DTYPE


def oracle_stereo_frame(width, height, nfeatures, seed):
    """Extract a synthetic pair with the oracle; returns dict with images, extractors, keys, descriptors."""
    L, R = synth.make_stereo_pair(width, height, seed)
    exL, exR = ob.Extractor(nfeatures), ob.Extractor(nfeatures)
    kL, dL, _ = exL.extract(L)
    kR, dR, _ = exR.extract(R)
    intr = synth.intrinsics(width, height)
    return dict(L=L, R=R, exL=exL, exR=exR, kL=kL, dL=dL, kR=kR, dR=dR, intr=intr)


def fisheye_frame_scenario(width, height, nfeatures, seed):
    """Two-camera (Nleft != -1) frame: left/right keypoints from the oracle on a synthetic pair, a
    brute-force left<->right match table, and local points visible in both cameras."""
    fr = oracle_stereo_frame(width, height, nfeatures, seed)
    m = ob.fisheye_match(fr["dL"], fr["dR"])
    l2r = m["matches"].astype(np.int32)
    r2l = np.full(len(fr["kR"]), -1, np.int32)
    for i, j in enumerate(l2r):
        if j >= 0:
            r2l[j] = i
    fr["l2r"], fr["r2l"] = l2r, r2l
    return fr


def padded_in_front(fr, n_total, seed, width, height):
    """A two-camera frame of exactly n_total keypoints without an extraction that large: the keypoints of `fr`
    (fisheye_frame_scenario's) with padding keypoints IN FRONT of them in each camera's arrays, half of the padding per camera (the
    odd one goes to the right camera).  A padding keypoint lies uniformly inside the 20 px border, at octave 0 .. 7, with a random
    angle, size 31 and a random descriptor; it has no left <-> right match.  The real keypoints keep their order, their match
    tables are shifted by the other camera's padding - so the real right-camera keypoints hold the highest indices of the frame.
    One seeded generator, host arrays only.  -> dict(kL, kR, dL, dR, l2r, r2l, padL, padR)"""
    rng = np.random.default_rng(seed)
    nl, nr = len(fr["kL"]), len(fr["kR"])
    pad = n_total - nl - nr
    assert pad >= 0, "the base frame has more keypoints than n_total"
    padL = pad // 2
    padR = pad - padL

    def camera(keys, desc, n):
        k = np.zeros(n, KP)
        k["x"] = rng.uniform(20.0, width - 20.0, n)
        k["y"] = rng.uniform(20.0, height - 20.0, n)
        k["size"] = 31.0
        k["angle"] = rng.uniform(0.0, 360.0, n)
        k["octave"] = rng.integers(0, 8, n)
        k["class_id"] = -1
        d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        return np.concatenate([k, keys]), np.concatenate([d, desc])
    kL, dL = camera(fr["kL"], fr["dL"], padL)
    kR, dR = camera(fr["kR"], fr["dR"], padR)
    l2r = np.concatenate([np.full(padL, -1, np.int32), np.where(fr["l2r"] >= 0, fr["l2r"] + padR, -1).astype(np.int32)])
    r2l = np.concatenate([np.full(padR, -1, np.int32), np.where(fr["r2l"] >= 0, fr["r2l"] + padL, -1).astype(np.int32)])
    return dict(kL=kL, kR=kR, dL=dL, dR=dR, l2r=l2r, r2l=r2l, padL=padL, padR=padR)


def two_camera_points(fr, sf, seed, M=1200, zero_obs_frac=0.2):
    rng = np.random.default_rng(seed)
    kL, kR, dL = fr["kL"], fr["kR"], fr["dL"]
    NL, NR = len(kL), len(kR)
    srcL = rng.integers(0, max(NL // 4, 1), M)
    srcR = rng.integers(0, max(NR // 4, 1), M)
    d = dL[srcL].copy()
    flips = rng.integers(0, 256, (M, 10))
    for k in range(10):
        mm = rng.random(M) < 0.5
        d[mm, flips[mm, k] // 8] ^= (1 << (flips[mm, k] % 8)).astype(np.uint8)
    both = rng.random(M)
    return dict(skip=(rng.random(M) < 0.04).astype(np.uint8), in_view=(both < 0.8).astype(np.uint8),
                in_view_r=(both > 0.3).astype(np.uint8),
                level=np.clip(kL["octave"][srcL] + rng.integers(0, 2, M), 0, len(sf) - 1).astype(np.int32),
                level_r=np.where(rng.random(M) < 0.1, -1,
                                 np.clip(kR["octave"][srcR] + rng.integers(0, 2, M), 0, len(sf) - 1)).astype(np.int32),
                view_cos=np.where(rng.random(M) < 0.5, 0.9995, 0.9).astype(np.float32),
                view_cos_r=np.where(rng.random(M) < 0.5, 0.9995, 0.9).astype(np.float32),
                proj_x=(kL["x"][srcL] + rng.normal(0, 2, M)).astype(np.float32),
                proj_y=(kL["y"][srcL] + rng.normal(0, 2, M)).astype(np.float32),
                proj_xr=(kR["x"][srcR] + rng.normal(0, 2, M)).astype(np.float32),
                proj_yr=(kR["y"][srcR] + rng.normal(0, 2, M)).astype(np.float32),
                descriptors=d,
                observations=np.where(rng.random(M) < zero_obs_frac, 0, rng.integers(1, 6, M)).astype(np.int32))


KB8_TRL = np.concatenate([np.eye(3), [[-0.101], [0.0], [0.0]]], 1).astype(np.float32)
KB8_TLR = (0.101, 0.0, 0.0)
_geometry_frames = {}


def geometry_frame(width, height, nfeatures, seed, scale_factor=1.2, nlevels=8, two_cameras=False, cache=True):
    """The frame the search tests are built on, extracted by the oracle with the pyramid (scale_factor, nlevels) - keypoint octaves
    lie in [0, nlevels) - and cached: a rectified stereo frame with its stereo match (fr["sm"]), or with two_cameras a frame with
    a brute-force left <-> right table (fisheye_frame_scenario's).  Carries the view's scale table (fr["sf"]) and
    Frame::mfLogScaleFactor (fr["log_sf"]): log(mfScaleFactor) stored as float."""
    key = (width, height, nfeatures, seed, scale_factor, nlevels, two_cameras)
    if not cache or key not in _geometry_frames:
        L, R = synth.make_stereo_pair(width, height, seed)
        exL, exR = ob.Extractor(nfeatures, scale_factor, nlevels), ob.Extractor(nfeatures, scale_factor, nlevels)
        kL, dL, _ = exL.extract(L)
        kR, dR, _ = exR.extract(R)
        fr = dict(L=L, R=R, exL=exL, exR=exR, kL=kL, dL=dL, kR=kR, dR=dR, intr=synth.intrinsics(width, height), w=width, h=height,
                  two_cameras=two_cameras, scale_factor=scale_factor, nlevels=nlevels, sf=ob.scale_factors(scale_factor, nlevels)[0],
                  log_sf=float(np.float32(np.log(np.float32(scale_factor)))))
        if two_cameras:
            l2r = ob.fisheye_match(dL, dR)["matches"].astype(np.int32)
            r2l = np.full(len(kR), -1, np.int32)
            for i, j in enumerate(l2r):
                if j >= 0:
                    r2l[j] = i
            fr["l2r"], fr["r2l"] = l2r, r2l
            fr["kb8_intr"] = dict(fx=KB8_CAM[0], fy=KB8_CAM[1], cx=KB8_CAM[2], cy=KB8_CAM[3])
        else:
            fr["sm"] = ob.stereo_match(exL, exR, kL, kR, dL, dR, fr["intr"]["mbf"], fr["intr"]["mb"])
        if not cache:
            return fr
        _geometry_frames[key] = fr
    return _geometry_frames[key]


def geometry_views(fr, bounds=None, uright=True, holder=None, device=True):
    """-> (oracle FrameView, device FrameView or None) of a geometry_frame under the image bounds `bounds` (default: (0, 0, w, h)),
    both with a fresh holder_obs.  Rectified frames: uright=False is the monocular frame.  Two-camera frames: KannalaBrandt8."""
    bounds = frame_bounds(fr["w"], fr["h"]) if bounds is None else bounds
    if fr["two_cameras"]:
        kw = dict(keys=fr["kL"], keys_right=fr["kR"], descriptors=np.concatenate([fr["dL"], fr["dR"]]), bounds=bounds,
                  left_to_right=fr["l2r"], right_to_left=fr["r2l"], cam_model=1, cam=list(KB8_CAM), Trl=KB8_TRL, holder_obs=holder)
    else:
        kw = dict(keys=fr["kL"], descriptors=fr["dL"], bounds=bounds, mbf=fr["intr"]["mbf"], mb=fr["intr"]["mb"],
                  uright=fr["sm"]["uright"] if uright else None, holder_obs=holder,
                  cam=[fr["intr"][k] for k in ("fx", "fy", "cx", "cy")])
    gF = None
    if device:
        from fasttrack_amd import orb
        gF = orb.FrameView(scale_factors=fr["sf"], **kw)
    return ob.FrameView(scale_factors_=fr["sf"], **kw), gF


def geometry_inputs(fr, seed, M=2500):
    """last-frame points and local map points (isInFrustum's) of a geometry_frame -> last, Tcw, pts, Rcw, tcw, tlr"""
    if fr["two_cameras"]:
        depth, intr, uright, tlr = np.zeros(len(fr["kL"]), np.float32), fr["kb8_intr"], None, KB8_TLR
    else:
        depth, intr, uright, tlr = fr["sm"]["depth"], fr["intr"], fr["sm"]["uright"], (0, 0, 0)
    last, Tcw = last_frame_scenario(fr["kL"], fr["dL"], uright, depth, intr, fr["w"], fr["h"], seed=seed)
    pts, Rcw, tcw = map_points_scenario(fr["kL"], fr["dL"], depth, intr, fr["nlevels"], fr["sf"], seed + 500, M=M)
    return last, Tcw, pts, Rcw, tcw, tlr


def lattice_views(lat, device=True):
    """-> (oracle FrameView, device FrameView or None) of a lattice_last_frame"""
    kw = dict(keys=lat["keys"], descriptors=lat["descriptors"], bounds=lat["bounds"], cam=lat["cam"])
    gF = None
    if device:
        from fasttrack_amd import orb
        gF = orb.FrameView(scale_factors=lat["scale_factors"], **kw)
    return ob.FrameView(scale_factors_=lat["scale_factors"], **kw), gF


def border_points(fr, bounds, last, pts, Tcw, Rcw, tcw, seed, n=60):
    """Appends n last-frame points and n local map points whose projections lie where the frame's bounds test and the image
    rectangle (0, 0, w, h) disagree - inside the bounds and outside the image, or the other way round - so that
    `u < mnMinX || u > mnMaxX` decides something whichever way the bounds differ from the image.  Each carries the descriptor,
    octave and angle of the keypoint nearest to its projection.  Rectified pinhole frames.  -> last, pts (new dicts)"""
    rng = np.random.default_rng(seed)
    w, h, intr, keys = fr["w"], fr["h"], fr["intr"], fr["kL"]
    fx, fy, cx, cy = [float(intr[k]) for k in ("fx", "fy", "cx", "cy")]
    lo_x, lo_y, hi_x, hi_y = min(bounds[0], 0.0), min(bounds[1], 0.0), max(bounds[2], w), max(bounds[3], h)

    def inside(u, v, b):
        return (u >= b[0]) & (u <= b[2]) & (v >= b[1]) & (v <= b[3])
    u, v = rng.uniform(lo_x, hi_x, 40 * n), rng.uniform(lo_y, hi_y, 40 * n)
    # (1.5 px clear of either border: the pose arithmetic below is float32, the selection float64)
    grow = lambda b, e: (b[0] - e, b[1] - e, b[2] + e, b[3] + e)
    img = (0.0, 0.0, float(w), float(h))
    pick = (inside(u, v, grow(bounds, -1.5)) & ~inside(u, v, grow(img, 1.5))) | (inside(u, v, grow(img, -1.5)) & ~inside(u, v, grow(bounds, 1.5)))
    u, v = u[pick][:2 * n], v[pick][:2 * n]
    assert len(u) == 2 * n, "bounds and image rectangle nearly coincide"
    near = np.argmin((keys["x"][None, :] - u[:, None]) ** 2 + (keys["y"][None, :] - v[:, None]) ** 2, axis=1)
    z = rng.uniform(2.0, 10.0, 2 * n)
    cam = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)      # in the camera frame of the pose it is seen from

    def to_world(R, t, Xc):
        return ((Xc - np.asarray(t, np.float64)[None, :]) @ np.asarray(R, np.float64)).astype(np.float32)   # R^T (x - t)
    a, b = slice(0, n), slice(n, 2 * n)
    la = dict(valid=np.ones(n, np.uint8), world_pos=to_world(Tcw[:, :3], Tcw[:, 3], cam[a]), descriptors=fr["dL"][near[a]],
              observations=rng.integers(0, 6, n).astype(np.int32), octave=keys["octave"][near[a]].astype(np.int32),
              angle=keys["angle"][near[a]].astype(np.float32))
    wp = to_world(Rcw, tcw, cam[b])
    Ow = -(np.asarray(Rcw, np.float64).T @ np.asarray(tcw, np.float64))
    PO = wp - Ow[None, :]
    dist = np.linalg.norm(PO, axis=1)
    max_d = (dist * fr["sf"][keys["octave"][near[b]]] * 1.05).astype(np.float32)
    pb = dict(world_pos=wp, normal=(PO / dist[:, None]).astype(np.float32), max_distance=max_d,
              min_distance=(max_d / fr["sf"][fr["nlevels"] - 1] * 0.9).astype(np.float32), skip=np.zeros(n, np.uint8),
              descriptors=fr["dL"][near[b]], observations=rng.integers(0, 6, n).astype(np.int32))
    return ({k: np.concatenate([last[k], la[k]]) for k in last}, {k: np.concatenate([pts[k], pb[k]]) for k in pts})


GEOMETRY_CASES = [("loose", 1.2, 8), ("tight", 1.2, 8), ("edge", 1.2, 8), ("tight", 1.5, 5), ("tight", 1.1, 12), ("tight", 2.0, 3),
                  ("tight", 1.2, 1)]   # every bounds at (1.2, 8), every pyramid at `tight`
GEOMETRY_FRAME = (640, 480, 1000, 31)   # width, height, nFeatures, seed of synth.make_stereo_pair
_geometry_cases = {}


def geometry_case(bounds_name, scale_factor, nlevels):
    """One parameter set of the geometry tests, cached: the frame (geometry_frame of GEOMETRY_FRAME), its bounds, last-frame points
    and local map points with border_points appended, and three local-point sets for the one-shot local-map search: dense
    (overlapping windows on the first sixth of the keypoints - the lowest octaves), sparse (all keypoints, hence every octave)
    and mono (dense, for the frame without mvuRight)."""
    key = (bounds_name, scale_factor, nlevels)
    if key not in _geometry_cases:
        w, h, nf, seed = GEOMETRY_FRAME
        fr = geometry_frame(w, h, nf, seed, scale_factor, nlevels)
        bounds = frame_bounds(w, h) if bounds_name == "default" else GEOMETRY_BOUNDS(w, h)[bounds_name]
        last, Tcw, pts, Rcw, tcw, tlr = geometry_inputs(fr, 4)
        if bounds_name != "default":
            last, pts = border_points(fr, bounds, last, pts, Tcw, Rcw, tcw, 9)
        ur = fr["sm"]["uright"]
        local = {name: local_points_scenario(fr["kL"], fr["dL"], fr["sf"], w, h, seed=70 + i, M=1500, uright=u, dense=dense)
                 for i, (name, u, dense) in enumerate((("dense", ur, True), ("sparse", ur, False), ("mono", None, True)))}
        _geometry_cases[key] = dict(fr=fr, bounds=bounds, last=last, Tcw=Tcw, pts=pts, Rcw=Rcw, tcw=tcw, tlr=tlr, local=local)
    return _geometry_cases[key]


def area_queries(bounds, nlevels, nq, seed):
    """nq windows: centres up to 60 px beyond the bounds on every side, radii 1 .. 120, level limits up to nlevels - 1 and beyond"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(bounds[0] - 60, bounds[2] + 60, nq).astype(np.float32)
    y = rng.uniform(bounds[1] - 60, bounds[3] + 60, nq).astype(np.float32)
    r = np.where(rng.random(nq) < 0.5, rng.choice([1.0, 2.5, 7.5, 15.0, 40.0, 120.0], nq), rng.uniform(1, 120, nq)).astype(np.float32)
    lo = rng.integers(-1, nlevels + 2, nq).astype(np.int32)
    hi = np.where(rng.random(nq) < 0.3, -1, lo + rng.integers(0, 4, nq)).astype(np.int32)
    right = (rng.random(nq) < 0.4).astype(np.uint8)
    for beyond in (x < bounds[0], x > bounds[2], y < bounds[1], y > bounds[3]):
        assert beyond.sum() >= 5
    assert r.min() == 1.0 and r.max() == 120.0 and (hi >= nlevels).any() and (lo >= nlevels).any()
    return x, y, r, lo, hi, right


def random_geometry(rng, width, height):
    """A frame geometry for the soaks: bounds = the image rectangle with every side moved by up to 45 px either way (fractional),
    a pyramid factor of {1.1, 1.2, 1.5, 2.0} and 1 .. 12 levels - fewer where the top level would get narrower than 96 px (the
    extractor needs its 19 px border twice and room for cells).  -> bounds, scale_factor, nlevels"""
    d = rng.uniform(-45.0, 45.0, 4)
    bounds = (float(d[0]), float(d[1]), float(width + d[2]), float(height + d[3]))
    factor = float(rng.choice([1.1, 1.2, 1.5, 2.0]))
    nlevels = int(rng.integers(1, 13))
    while nlevels > 1 and min(width, height) / factor ** (nlevels - 1) < 96:
        nlevels -= 1
    return bounds, factor, nlevels

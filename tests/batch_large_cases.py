"""Frames beyond the LDS last-writer tables of k_resolve_batch / k_replay_batch, and directed chunk hand-over cases (cached per
process; shared by test_batch_large_cpu.py - the oracle alone - and test_gpu_batch_large.py).

Where the per-keypoint last-writer tables live is decided by the largest frame of a batch (csrc/tracked_batch.cpp):
    F.N <= RESOLVE_LDS_MAX              both tables in LDS
    RESOLVE_LDS_MAX < F.N <= REPLAY_LDS_MAX   k_resolve_batch's table in HBM, k_replay_batch's in LDS
    F.N > REPLAY_LDS_MAX                both in HBM
REGIMES holds the two sizes on either side of each threshold.  A regime's batch is three two-camera KannalaBrandt8 frames: the
base frame (fisheye_frame_scenario, 512x512, nFeatures 2000: ~1 960 + 1 980 keypoints) padded in front to the regime's size
(scenarios.padded_in_front), the base frame itself, and the base frame cut to (300, 300) keypoints - the small frames go
through the same kernel variants as the large one.

Every frame gets POINTS last-frame points and POINTS local map points: CHUNKS chunks of the 64 points k_resolve_batch walks at a
time.  The points are built on the REAL keypoints (scenarios.last_frame_scenario on the real left keypoints, map_points_scenario
for the local map: ft_tracked_batch_track_local_map takes world points and runs isInFrustum itself, so the local points are world
points and not projections).  The directed cases (PATTERNS) put copies of HOT points at positions 64 c + 3 .. 64 c + 42 of
every chunk c, with Observations() set per chunk: what a copy does depends on what the copies in the chunks in front of it left
in the last-writer table.  "plain" has no copies."""
import os

import numpy as np

from oracle import binding as ob
from tests import scenarios as sc

RESOLVE_LDS_MAX = 12288   # tracked_batch.cpp: `c.shInts <= 12288` (callResolve)
REPLAY_LDS_MAX = 15360    # tracked_batch.cpp: `maxN <= 15360` (replayShared)
REGIMES = (RESOLVE_LDS_MAX, RESOLVE_LDS_MAX + 1, REPLAY_LDS_MAX, REPLAY_LDS_MAX + 1)
TRACKED_BATCH_CPP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fasttrack_amd", "csrc", "tracked_batch.cpp")

W = H = 512
NFEATURES, BASE_SEED = 2000, 10
TH = 15.0
LOG_SF = float(np.float32(np.log(np.float32(1.2))))
CHUNK, CHUNKS, HOT = 64, 5, 40
POINTS = CHUNK * CHUNKS   # 320
CANDIDATES = 4 * POINTS   # local map points drawn per frame, of which POINTS are kept
# Observations() of the hot copies, per chunk
PATTERNS = {"alternate": (0, 3, 0, 3, 0),   # a copy that locks behind one that does not, and the other way round
            "all3": (3, 3, 3, 3, 3),        # every later copy is locked out and takes its second best
            "all0": (0, 0, 0, 0, 0)}        # every later copy overwrites: a chain through all five chunks
PATTERN_SEED = {"plain": 100, "alternate": 101, "all3": 102, "all0": 103}
CACHE_CAP = 511           # csrc/ft_search.h FT_CACHE_CAP: a longer candidate list makes k_resolve_batch give up on the frame
HIGH = 2000               # "the frame's highest indices": the real right-camera keypoints of a padded frame
HELD_FRACTION = 0.3       # the padded frame of the largest regime: keypoints held before the call, Observations() 0 / 1 / 2

_cache = {}


def scale_factors():
    return ob.scale_factors(1.2, 8)[0]


def base_frame():
    if "base" not in _cache:
        _cache["base"] = sc.fisheye_frame_scenario(W, H, NFEATURES, BASE_SEED)
    return _cache["base"]


def frame_arrays(which, n_total=None):
    """the arrays of one frame of a regime's batch: "padded" (to n_total keypoints), "whole", "cut" -> padded_in_front's dict"""
    key = ("arrays", which, n_total if which == "padded" else None)
    if key not in _cache:
        fr = base_frame()
        if which == "padded":
            a = sc.padded_in_front(fr, n_total, n_total, W, H)
        else:
            nl, nr = (300, 300) if which == "cut" else (len(fr["kL"]), len(fr["kR"]))
            a = dict(kL=fr["kL"][:nl], kR=fr["kR"][:nr], dL=fr["dL"][:nl], dR=fr["dR"][:nr],
                     l2r=np.where(fr["l2r"][:nl] < nr, fr["l2r"][:nl], -1).astype(np.int32),
                     r2l=np.where(fr["r2l"][:nr] < nl, fr["r2l"][:nr], -1).astype(np.int32), padL=0, padR=0)
        if which == "padded" and n_total == REGIMES[-1]:
            rng = np.random.default_rng(n_total + 1)
            a["holder"] = np.where(rng.random(n_total) < HELD_FRACTION, rng.integers(0, 3, n_total), -1).astype(np.int32)
        _cache[key] = a
    return _cache[key]


def frame_kw(a):
    """FrameView arguments (the oracle's and the device's alike) of a frame's arrays; holder_obs is copied by the views"""
    return dict(keys=a["kL"], keys_right=a["kR"], descriptors=np.concatenate([a["dL"], a["dR"]]), bounds=sc.frame_bounds(W, H),
                left_to_right=a["l2r"], right_to_left=a["r2l"], cam_model=1, cam=list(sc.KB8_CAM), Trl=sc.KB8_TRL,
                holder_obs=a.get("holder"))


def _place(hot, rest):
    """-> source index of each of the POINTS positions - chunk c holds a copy of hot[h] at position 64 c + 3 + h, the other
    positions take `rest` in order - and which positions hold a hot copy"""
    rest = iter(rest)
    idx, is_hot = np.empty(POINTS, np.int64), np.zeros(POINTS, bool)
    for p in range(POINTS):
        j = p % CHUNK
        if 3 <= j < 3 + HOT:
            idx[p], is_hot[p] = hot[j - 3], True
        else:
            idx[p] = next(rest)
    return idx, is_hot


def _pattern_obs(obs, is_hot, pattern):
    obs = obs.copy()
    if pattern != "plain":
        per_chunk = np.repeat(np.asarray(PATTERNS[pattern], np.int32), CHUNK)
        obs[is_hot] = per_chunk[is_hot]
    return obs


def local_list_bounds(a, seen, skip):
    """an upper bound of the candidates in every local map point's left and right window in frame `a`: the keypoints of the level
    band inside the box of Frame::GetFeaturesInArea as SearchByProjection calls it (src/ORBmatcher.cc:76-90, 151-160; the grid
    cells can only drop some of them).  `seen` = isInFrustum's fields -> int array [M, 2]"""
    sf = scale_factors()
    n = np.zeros((len(skip), 2), np.int64)
    for cam, (keys, view, lv, cos, x, y) in enumerate(((a["kL"], "in_view", "level", "view_cos", "proj_x", "proj_y"),
                                                       (a["kR"], "in_view_r", "level_r", "view_cos_r", "proj_xr", "proj_yr"))):
        kx, ky, ko = keys["x"], keys["y"], keys["octave"]
        for p in np.flatnonzero((np.asarray(skip) == 0) & (seen[view] != 0) & (seen[lv] >= 0)):
            level = int(seen[lv][p])
            r = np.float32(2.5 if seen[cos][p] > np.float32(0.998) else 4.0) * np.float32(TH) * sf[level]
            n[p, cam] = np.count_nonzero((np.abs(kx - seen[x][p]) < r) & (np.abs(ky - seen[y][p]) < r) & (ko >= level - 1) & (ko <= level))
    return n


def frame_inputs(which, pattern):
    """last-frame points, Tcw, local map points, Rcw, tcw of frame `which` under `pattern` (the padded frame's are built on its
    real keypoints, whatever the padding: the same for every regime)"""
    key = ("inputs", which, pattern)
    if key in _cache:
        return _cache[key]
    a = frame_arrays("cut" if which == "cut" else "whole")
    kL, dL = a["kL"], a["dL"]
    seed = PATTERN_SEED[pattern] + 1000 * ("padded", "whole", "cut").index(which)
    rng = np.random.default_rng(seed)
    intr = dict(fx=sc.KB8_CAM[0], fy=sc.KB8_CAM[1], cx=sc.KB8_CAM[2], cy=sc.KB8_CAM[3])
    depth = np.zeros(len(kL), np.float32)
    # last frame: every point valid, 10 % of them with an angle 40 - 320 degrees off (the rotation histogram removes matches)
    full, Tcw = sc.last_frame_scenario(kL, dL, None, depth, intr, W, H, seed=seed)
    n_rest = POINTS - CHUNKS * HOT
    if pattern == "plain":
        idx, is_hot = rng.choice(len(kL), POINTS, replace=len(kL) < POINTS), np.zeros(POINTS, bool)
    else:
        sel = rng.choice(len(kL), HOT + n_rest, replace=False)
        idx, is_hot = _place(sel[:HOT], sel[HOT:])
    last = {k: v[idx].copy() for k, v in full.items()}
    last["valid"][:] = 1
    last["observations"] = _pattern_obs(last["observations"], is_hot, pattern)
    off = rng.random(POINTS) < 0.1
    last["angle"][off] = ((last["angle"][off] + rng.uniform(40.0, 320.0, int(off.sum()))) % 360.0).astype(np.float32)
    # local map: POINTS of CANDIDATES points; the hot copies are taken from those the frame (its real keypoints, nothing held) matches
    # with BOTH cameras when every candidate is searched once - copies of a point no camera sees would hand nothing over
    cand, Rcw, tcw = sc.map_points_scenario(kL, dL, depth, intr, 8, scale_factors(), seed + 500, M=CANDIDATES)
    oF = ob.FrameView(scale_factors_=scale_factors(), **frame_kw(a))
    seen = ob.is_in_frustum(oF, ob.make_pose(Rcw, tcw, sc.KB8_TLR), cand, 0.5, LOG_SF)
    once = ob.search_local_points(oF, sc.local_points_from_frustum(seen, cand), TH)
    both = (once["best_idx"] >= 0) & (once["best_dist"] <= 100) & (once["best_idx_r"] >= 0) & (once["best_dist_r"] <= 100)
    # ... and every candidate's lists fit the candidate cache on every frame it is searched on, so that k_resolve_batch gives up
    # on no frame (a padded frame has ~6 000 padding keypoints per camera: the window of a high level holds thousands)
    on = [frame_arrays("padded", n) for n in REGIMES] if which == "padded" else [a]
    fits = np.all([local_list_bounds(f, seen, cand["skip"]).max(axis=1) <= CACHE_CAP for f in on], axis=0)
    assert fits.sum() >= POINTS, "too few local map points with candidate lists inside the cache"
    pool = np.flatnonzero(fits)
    pool = pool[np.argsort(~(both[pool] & (cand["skip"][pool] == 0)), kind="stable")]
    if pattern == "plain":
        idx2 = rng.permutation(np.concatenate([pool[:HOT], rng.permutation(pool[HOT:])[:POINTS - HOT]]))
        is_hot2 = np.zeros(POINTS, bool)
    else:
        idx2, is_hot2 = _place(pool[:HOT], rng.permutation(pool[HOT:])[:n_rest])
    pts = {k: v[idx2].copy() for k, v in cand.items()}
    pts["skip"][is_hot2] = 0
    pts["observations"] = _pattern_obs(pts["observations"], is_hot2, pattern)
    _cache[key] = (last, Tcw, pts, Rcw, tcw)
    return _cache[key]


def oracle_sequence(a, last, Tcw, pts, Rcw, tcw, check_orientation=True, th=TH):
    """the reference's sequence on one frame -> o1, ofr, o2, oF (oF.holder_obs: the final one)"""
    oF = ob.FrameView(scale_factors_=scale_factors(), **frame_kw(a))
    o1 = ob.search_last_frame(oF, last, Tcw, th, False, False, check_orientation)
    ofr = ob.is_in_frustum(oF, ob.make_pose(Rcw, tcw, sc.KB8_TLR), pts, 0.5, LOG_SF)
    o2 = ob.search_local_points(oF, sc.local_points_from_frustum(ofr, pts), th)
    return o1, ofr, o2, oF


def regime_case(n_total, pattern):
    """-> list of three dicts (padded, whole, cut): arrays a, inputs (last, Tcw, pts, Rcw, tcw), oracle (o1, ofr, o2, oF)"""
    key = ("case", n_total, pattern)
    if key not in _cache:
        frames = []
        for which in ("padded", "whole", "cut"):
            ckey = ("frame", which, n_total if which == "padded" else None, pattern)
            if ckey not in _cache:   # (the small frames are the same in every regime)
                a = frame_arrays(which, n_total)
                inputs = frame_inputs(which, pattern)
                _cache[ckey] = dict(which=which, a=a, inputs=inputs, oracle=oracle_sequence(a, *inputs))
            frames.append(_cache[ckey])
        _cache[key] = frames
    return _cache[key]


def owned(assign, n_points):
    """per point: the sorted keypoints whose final assignment is that point"""
    own = [[] for _ in range(n_points)]
    for kp in np.flatnonzero(assign >= 0):
        own[int(assign[kp])].append(int(kp))
    return own


def chunk_dependent_points(a, last, Tcw):
    """last-frame points whose result in the whole search (the keypoints they end up owning, orientation filter off: the claims
    alone) differs from their result when their chunk is searched alone (every other chunk's `valid` set to 0)"""
    def run(l):
        oF = ob.FrameView(scale_factors_=scale_factors(), **frame_kw(a))
        return owned(ob.search_last_frame(oF, l, Tcw, TH, False, False, False)["assign"], POINTS)
    whole = run(last)
    n = 0
    for c in range(CHUNKS):
        alone = {k: v.copy() for k, v in last.items()}
        alone["valid"][:] = 0
        alone["valid"][CHUNK * c:CHUNK * (c + 1)] = last["valid"][CHUNK * c:CHUNK * (c + 1)]
        own = run(alone)
        n += sum(whole[p] != own[p] for p in range(CHUNK * c, CHUNK * (c + 1)))
    return n


def conditions(n_total, pattern):
    """what keeps the padded frame's case from being vacuous, measured on the oracle alone -> dict of counts"""
    fr = regime_case(n_total, pattern)[0]
    a, (last, Tcw, pts, Rcw, tcw), (o1, ofr, o2, oF) = fr["a"], fr["inputs"], fr["oracle"]
    loose = oracle_sequence(a, last, Tcw, pts, Rcw, tcw, check_orientation=False)[0]
    N, nleft = oF.N, oF.Nleft
    return dict(last_matches=int(o1["n"]), removed=int(loose["n"] - o1["n"]),
                high=int((o1["assign"][N - HIGH:] >= 0).sum()),
                chunk_dependent=chunk_dependent_points(a, last, Tcw) if pattern != "plain" else None,
                local_matches=int(o2["n"]), local_right=int((o2["assign"][nleft:] >= 0).sum()),
                longest_local_list=int(local_list_bounds(a, ofr, sc.local_points_from_frustum(ofr, pts)["skip"]).max()))

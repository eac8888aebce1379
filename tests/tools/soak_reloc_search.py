#!/usr/bin/env python3
"""Long randomized parity run of ORBmatcher::SearchByProjection(Frame, KeyFrame, sAlreadyFound, th, ORBdist) on an MI355X (not part
of the test suite): ft_search_keyframe_projection and ft_tracked_frame_search_keyframe_projection against the restatement
(tests/reloc_search_ref.py).
usage: tests/tools/soak_reloc_search.py [--trials N] [--seed S]

A trial draws a frame size, a feature count, a scene, image bounds and a pyramid (tests/scenarios.py random_geometry), extracts the
frame with the oracle and builds the keyframe's points as tests/reloc_cases.py does (two per keypoint, random ranges, 85 % valid,
a random share of the keypoints held on entry); th in 1 .. 15, ORBdist in 30 .. 120, orientation check on or off, pinhole or
KannalaBrandt8, and now and then descriptors from a small dictionary (ties everywhere).  The resident frame is searched twice
as Tracking::Relocalization does (the second call on the occupancy the first left).  assign, nmatches, holder_obs, bestDist and
bestIdx2 must be equal.  Prints one line per failure and a summary; exit code 1 on any mismatch."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb, synth  # noqa: E402
from oracle import binding as ob  # noqa: E402
from tests import reloc_cases as rc  # noqa: E402
from tests import reloc_search_ref as ref  # noqa: E402
from tests import scenarios as sc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=100)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
ctx = orb.Context(0)
tf = orb.TrackedFrame(ctx, 8192, 4096)
calls = mismatches = 0
tot = dict(changed_by_locks=0, locked_skips=0, removed_by_histogram=0, accepted=0, capacity=0)
t0 = time.time()


def compare(tag, g, r, holder, with_best):
    global calls, mismatches
    calls += 1
    bad = [k for k in (("assign", "best_dist", "best_idx") if with_best else ("assign",)) if not np.array_equal(g[k], r[k])]
    if g["n"] != r["n"]:
        bad.append("n")
    if not np.array_equal(holder, r["holder_obs"]):
        bad.append("holder_obs")
    if bad:
        mismatches += 1
        print(f"MISMATCH {tag}: {bad}")


for trial in range(args.trials):
    w, h = [(320, 240), (640, 480), (752, 480), (512, 512)][int(rng.integers(0, 4))]
    nf, seed = int(rng.choice([300, 1000, 2000])), int(rng.integers(0, 1 << 30))
    bounds, factor, nlevels = sc.random_geometry(rng, w, h)
    img = synth.make_image(w, h, seed % 1000)
    keys, desc, _ = ob.Extractor(nf, factor, nlevels).extract(img)
    if len(keys) < 20:
        continue
    sf = ob.scale_factors(factor, nlevels)[0]
    log_sf = float(np.float32(np.log(np.float32(factor))))
    kb8 = rng.random() < 0.3
    cam = [c * w / 512.0 for c in sc.KB8_CAM[:4]] + sc.KB8_CAM[4:] if kb8 else [synth.intrinsics(w, h)[k] for k in ("fx", "fy", "cx", "cy")]
    intr = dict(fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3])
    kf, (q, t) = rc.keyframe_points(keys, desc, sf, intr, w, h, seed % 100000, kb8_cam=cam if kb8 else None)
    if rng.random() < 0.2:   # a dictionary of a few descriptors on both sides: equal distances everywhere
        dic = rng.integers(0, 256, (int(rng.integers(2, 12)), 32), dtype=np.uint8)
        desc = dic[rng.integers(0, len(dic), len(keys))]
        kf["descriptors"] = dic[rng.integers(0, len(dic), len(kf["valid"]))]
    holder = np.where(rng.random(len(keys)) < rng.uniform(0, 0.5), rng.integers(0, 3, len(keys)), -1).astype(np.int32)
    th, od, ori = float(rng.integers(1, 16)), int(rng.integers(30, 121)), bool(rng.random() < 0.7)
    kw = dict(keys=keys, descriptors=desc, bounds=bounds, cam_model=int(kb8), cam=cam, holder_obs=holder)
    oF, gF = ob.FrameView(scale_factors_=sf, **kw), orb.FrameView(scale_factors=sf, **kw)
    T, gT = ob.SE3(q, t), orb.SE3(q, t)
    tag = f"trial {trial} {w}x{h} nf {nf} seed {seed} bounds {bounds} pyramid {factor}/{nlevels} kb8 {kb8} th {th} ORBdist {od} ori {ori}"
    r = ref.search_by_projection(oF, kf, T, log_sf, th, od, ori)
    try:
        g = orb.KernelController.search_keyframe_projection(ctx, gF, kf, gT, log_sf, th, od, ori)
    except orb.FastTrackError as e:
        if e.status != -4:
            raise
        tot["capacity"] += 1
        continue
    compare(tag + " view", g, r, gF.holder_obs, True)
    tf.upload(orb.FrameView(scale_factors=sf, **kw))
    g1 = tf.search_keyframe_projection(kf, gT, log_sf, th, od, ori)
    compare(tag + " resident", g1, r, tf.holder_obs(), False)
    found = np.zeros(len(kf["valid"]), bool)
    found[r["assign"][r["assign"] >= 0]] = True
    kf2 = dict(kf, valid=(kf["valid"].astype(bool) & ~found).astype(np.uint8))
    oF.holder_obs[:] = r["holder_obs"]
    r2 = ref.search_by_projection(oF, kf2, T, log_sf, 3.0, 64, ori)
    g2 = tf.search_keyframe_projection(kf2, gT, log_sf, 3.0, 64, ori)
    compare(tag + " resident, second call", g2, r2, tf.holder_obs(), False)
    for k in ("changed_by_locks", "locked_skips", "removed_by_histogram", "accepted"):
        tot[k] += r["stats"][k] + r2["stats"][k]
print(f"soak_reloc_search: {args.trials} trials (seed {args.seed}), {calls} calls, {mismatches} mismatches, {tot}, {time.time() - t0:.0f} s, "
      f"{orb.version()}")
sys.exit(1 if mismatches else 0)

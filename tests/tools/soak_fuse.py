#!/usr/bin/env python3
"""Long randomized parity run of ORBmatcher::Fuse on an MI355X (not part of the test suite): ft_fuse_search against the
restatement (tests/fuse_ref.py).
usage: tests/tools/soak_fuse.py [--trials N] [--seed S]

A trial draws a frame (pinhole of several sizes and feature counts, KannalaBrandt8 with one camera, with two - left or right),
the points of tests/fuse_cases.py on it under a fresh seed, 1 .. 4 targets on that frame with poses of their own (the first the
case's, the others random steps), th in {2, 3, 4, 6, 10}, the overload (SE3 with the chi-square test or Sim3 without) per
target, valid or NULL.  bestIdx, bestDist, stage and n_found must be equal for every target, and the batched call must equal the
single calls.  Prints one line per failure and a summary; exit code 1 on any mismatch."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from oracle import binding as ob  # noqa: E402
from tests import fuse_cases as fc  # noqa: E402
from tests import fuse_ref as ref  # noqa: E402
from tests import reloc_cases as rc  # noqa: E402
from tests import reloc_search_ref as rref  # noqa: E402
from tests import scenarios as sc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=40)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
ctx = orb.Context(0)
FRAMES = ["pinhole:320x240:500:5", "pinhole:640x480:1000:3", "pinhole:320x240:300:8", "kb8mono", "kb8two", "kb8two:right",
          "geometry:tight:1.2:8", "geometry:loose:1.1:12"]
calls = targets_run = mismatches = 0
tot = dict(points=0, found=0, chi=0, changed=0, ties=0, stages=[0] * 7)
t0 = time.time()
for trial in range(args.trials):
    name = FRAMES[int(rng.integers(0, len(FRAMES)))]
    case = fc.random_case(name)
    base = rc.random_case(name.split(":right")[0])
    seed = int(rng.integers(0, 1 << 30))
    if case["right"]:
        kf, _ = rc.keyframe_points(base["fr"]["kR"], base["fr"]["dR"], base["fr"]["sf"], base["fr"]["kb8_intr"], 512, 512, seed % 1000, kb8_cam=sc.KB8_CAM)
    else:
        kf = base["kf"]
    pts, valid, _ = fc.fuse_points(kf, case["Tcw"], seed)
    oF, gF = case["view"]()
    specs = []
    for k in range(int(rng.integers(1, 5))):
        Tcw = case["Tcw"] if k == 0 else ob.SE3(*sc.random_se3(rng))
        specs.append(dict(Tcw=Tcw, Ow=rref.camera_centre(Tcw), th=float(rng.choice([2.0, 3.0, 4.0, 6.0, 10.0])), check=bool(rng.random() < 0.6),
                          valid=valid if rng.random() < 0.8 else None))
    tg = [dict(kf=gF, Tcw=orb.SE3(s["Tcw"].q, s["Tcw"].t), Ow=s["Ow"], log_scale_factor=case["log_sf"], th=s["th"], right=case["right"],
               cam2=case["cam2"], valid=s["valid"], check_reprojection=s["check"]) for s in specs]
    g = orb.fuse_search(ctx, pts, tg)
    calls += 1
    for k, s in enumerate(specs):
        r = ref.fuse(oF, pts, s["Tcw"], s["Ow"], case["log_sf"], s["th"], case["right"], case["cam2"], s["valid"], s["check"])
        one = orb.fuse_search(ctx, pts, [tg[k]])
        targets_run += 1
        bad = [f for f in ("best_idx", "best_dist", "stage") if not np.array_equal(g[f][k], r[f])]
        bad += ["n_found"] if int(g["n_found"][k]) != r["n_found"] else []
        bad += ["single != batched"] if not all(np.array_equal(one[f][0], g[f][k]) for f in ("best_idx", "best_dist", "stage")) else []
        if bad:
            mismatches += 1
            print(f"MISMATCH trial {trial} {name} seed {seed} target {k} th {s['th']} check {s['check']}: {bad}")
        st = r["stats"]
        tot["points"] += len(valid)
        tot["found"] += r["n_found"]
        tot["chi"] += st["chi_stereo"] + st["chi_mono"]
        tot["changed"] += st["changed_by_chi"]
        tot["ties"] += st["ties"]
        tot["stages"] = [a + b for a, b in zip(tot["stages"], st["stages"])]
print(f"fuse soak: seed {args.seed}, {args.trials} trials, {calls} batched calls, {targets_run} targets, {mismatches} mismatches; the restatement saw "
      f"{tot['points']} points, exits 0 .. 6 {tot['stages']}, {tot['found']} with bestDist <= 50, {tot['chi']} chi-square rejections "
      f"({tot['changed']} points whose best changed), {tot['ties']} ties; {orb.version()} on {ctx.device_name}, {time.time() - t0:.0f} s")
sys.exit(1 if mismatches else 0)

#!/usr/bin/env python3
"""Long randomized parity run of ft_pose_optimization on an MI355X (not part of the test suite) against the restatement
(tests/pose_opt_ref.py).
usage: tests/tools/soak_pose_opt.py [--trials N] [--seed S] [--out profiles/pose_opt_soak.json]

A trial draws 1 .. 8 frames: a camera form (pinhole mono / stereo / mixed, KannalaBrandt8 with one or two cameras), 3 .. 700
observations among up to twice as many keypoints, 0 .. 1.5 level sigmas of pixel noise, 0 .. 30 % gross outliers, an initial pose up
to 0.1 rad / 0.3 m off.  The frames go to the device in one call.  mvbOutlier, the return value and the integers of the trace must
be equal, the pose within POSE_TOL and currentChi within the same relative tolerance; the run also counts the frames that are equal
bit for bit.  A frame with an edge whose chi2 lies within 1e-6 (relative) of its threshold in any round is skipped; the share
skipped is reported and fails the run above 1 %.  (The Levenberg-Marquardt margin of the restatement is reported, not used: it is
at the round-off in every converging run, see test_pose_opt_cpu.py.)  Exit code 1 on any mismatch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from tests import pose_opt_cases as pc  # noqa: E402
from tests import pose_opt_ref as ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=40)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--out", default=None)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
ctx = orb.Context(0)
frames = skipped = mismatches = bit_equal = lm_clear = 0
t0 = time.time()
for trial in range(args.trials):
    batch = []
    for _ in range(int(rng.integers(1, 9))):
        n_obs = int(rng.integers(3, 701))
        batch.append(pc.frame.__wrapped__(pc.FORMS[int(rng.integers(0, 5))], int(rng.integers(0, 1 << 30)), n_obs, n_obs + int(rng.integers(0, n_obs + 1)),
                                          noise=float(rng.uniform(0, 1.5)), outliers=float(rng.uniform(0, 0.3)),
                                          perturb=(float(rng.uniform(0, 0.1)), float(rng.uniform(0, 0.3)))))
    got = orb.pose_optimization(ctx, [pc.to_device(orb, F) for F in batch])
    for i, (F, g) in enumerate(zip(batch, got)):
        want = ref.pose_optimization(F)
        frames += 1
        lm_clear += want["lm_margin"] >= pc.MARGIN
        if want["edge_margin"] < pc.MARGIN:
            skipped += 1
            continue
        bad = []
        if not np.array_equal(g["outlier"], want["outlier"]) or g["ret"] != want["ret"]:
            bad.append("flags")
        if [t[:2] for t in g["trace"]] != [t[:2] for t in want["trace"]]:
            bad.append("trace")
        if not (pc.pose_close(g["Tcw"][0], want["Tcw"][0]) and pc.pose_close(g["Tcw"][1], want["Tcw"][1])):
            bad.append("pose")
        if any(abs(a[2] - b[2]) > pc.CHI_RTOL * abs(b[2]) for a, b in zip(g["trace"], want["trace"])):
            bad.append("chi")
        bit_equal += (not bad and np.array_equal(g["Tcw"][0], want["Tcw"][0]) and np.array_equal(g["Tcw"][1], want["Tcw"][1]) and
                      [t[2] for t in g["trace"]] == [t[2] for t in want["trace"]])
        if bad:
            mismatches += 1
            print(f"MISMATCH trial {trial} frame {i} {F['form']} {want['n_edges']} edges: {bad} {g['trace']} {want['trace']}")
share = skipped / max(frames, 1)
summary = dict(seed=args.seed, trials=args.trials, frames=frames, skipped=skipped, skipped_share=round(share, 4), mismatches=mismatches,
               bit_equal=bit_equal, lm_margin_clear=int(lm_clear), library=orb.version(), device=ctx.device_name, seconds=round(time.time() - t0, 1))
print(f"pose-optimization soak: {json.dumps(summary)}")
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(summary) + "\n")
sys.exit(1 if mismatches or share > 0.01 else 0)

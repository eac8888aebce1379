#!/usr/bin/env python3
"""Long randomized parity run of ORBmatcher::SearchByProjection(pKF, Scw, ...) on an MI355X (not part of the test suite):
ft_search_keyframe_sim3 against the restatement (tests/sim3_search_ref.py).
usage: tests/tools/soak_sim3_search.py [--trials N] [--seed S]

A trial draws a frame (pinhole of several sizes and feature counts, KannalaBrandt8 with one and two cameras, shifted bounds, other
pyramids), the points of tests/sim3_cases.py on it under a fresh seed, 1 .. 4 jobs with poses of their own (the first the case's,
the others random steps), th in {3, 5, 8, 12}, ratio in {0.6, 1.0, 1.5, 2.0}, either projection form, valid or NULL, vpMatched as
the case's, all free, or what the previous job left.  matched, point_keypoint, stage and n_matches must be equal for every job, and
the batched call must equal the single calls.  Prints one line per failure and a summary; exit code 1 on any mismatch."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from oracle import binding as ob  # noqa: E402
from tests import reloc_cases as rc  # noqa: E402
from tests import reloc_search_ref as rref  # noqa: E402
from tests import scenarios as sc  # noqa: E402
from tests import sim3_cases as s3  # noqa: E402
from tests import sim3_search_ref as ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=40)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
ctx = orb.Context(0)
FRAMES = ["pinhole:320x240:500:5", "pinhole:640x480:1000:3", "pinhole:320x240:300:8", "kb8mono", "kb8two", "geometry:tight:1.2:8",
          "geometry:loose:1.1:12", "geometry:tight:2.0:2"]
FIELDS = ("matched", "point_keypoint", "stage")
calls = jobs_run = mismatches = 0
tot = dict(points=0, matches=0, walk=0, changed=0, held=0, past_top=0, stages=[0] * 8)
t0 = time.time()
for trial in range(args.trials):
    name = FRAMES[int(rng.integers(0, len(FRAMES)))]
    base = rc.random_case(name)
    seed = int(rng.integers(0, 1 << 30))
    pts, valid, _, matched0 = s3.sim3_points(base, seed)
    oF, gF = base["view"]()
    specs, entry = [], matched0
    for k in range(int(rng.integers(1, 5))):
        Tcw = base["Tcw"] if k == 0 else ob.SE3(*sc.random_se3(rng))
        pick = rng.random()
        s = dict(Tcw=Tcw, Ow=rref.camera_centre(Tcw), th=int(rng.choice([3, 5, 8, 12])), ratio=float(rng.choice([0.6, 1.0, 1.5, 2.0])),
                 hand=bool(rng.random() < 0.5), valid=valid if rng.random() < 0.8 else None,
                 matched=entry if pick < 0.5 else (matched0 if pick < 0.8 else np.full(len(matched0), -1, np.int32)))
        s["ref"] = ref.search(oF, pts, s["Tcw"], s["Ow"], base["log_sf"], s["th"], s["ratio"], s["matched"], s["valid"], s["hand"])
        s["compacted"] = ref.search_compacted(oF, pts, s["Tcw"], s["Ow"], base["log_sf"], s["th"], s["ratio"], s["matched"], s["valid"], s["hand"])
        entry = s["ref"]["matched"]
        specs.append(s)
    jobs = [dict(points=pts, Tcw=orb.SE3(s["Tcw"].q, s["Tcw"].t), Ow=s["Ow"], log_scale_factor=base["log_sf"], th=s["th"], ratio_hamming=s["ratio"],
                 hand_pinhole=s["hand"], valid=s["valid"], matched=s["matched"]) for s in specs]
    g = orb.search_keyframe_sim3(ctx, gF, jobs)
    calls += 1
    for k, s in enumerate(specs):
        r = s["ref"]
        one = orb.search_keyframe_sim3(ctx, gF, [jobs[k]])[0]
        jobs_run += 1
        bad = [f for f in FIELDS if not np.array_equal(g[k][f], r[f])]
        bad += ["n_matches"] if g[k]["n_matches"] != r["n_matches"] else []
        bad += ["single != batched"] if not all(np.array_equal(one[f], g[k][f]) for f in FIELDS) else []
        bad += ["restatements differ"] if not all(np.array_equal(s["compacted"][f], r[f]) for f in FIELDS) else []
        if bad:
            mismatches += 1
            print(f"MISMATCH trial {trial} {name} seed {seed} job {k} th {s['th']} ratio {s['ratio']} hand {s['hand']}: {bad}")
        st = r["stats"]
        tot["points"] += len(valid)
        tot["matches"] += r["n_matches"]
        tot["walk"] += st["walk"]
        tot["changed"] += st["changed_by_locks"]
        tot["held"] += st["held_on_entry"]
        tot["past_top"] += s["compacted"]["stats"]["past_top"]
        tot["stages"] = [a + b for a, b in zip(tot["stages"], st["stages"])]
print(f"sim3 soak: seed {args.seed}, {args.trials} trials, {calls} batched calls, {jobs_run} jobs, {mismatches} mismatches; the restatement saw "
      f"{tot['points']} points, exits 0 .. 7 {tot['stages']}, {tot['walk']} entering the walk, {tot['matches']} writes, {tot['changed']} changed by "
      f"earlier writes, {tot['held']} looks at keypoints held on entry, {tot['past_top']} points past their top record; "
      f"{orb.version()} on {ctx.device_name}, {time.time() - t0:.0f} s")
sys.exit(1 if mismatches else 0)

#!/usr/bin/env python3
"""Latency of ft_search_keyframe_sim3 on an MI355X (not part of the test suite): a 752 x 480 keyframe extracted with nFeatures 2000
against the points of tests/sim3_cases.py on it (three per keypoint: about 6 000, a covisibility window's worth), with the
parameter pairs of Loop Closing - (th 8, ratio 1.5) written out, (5, 1.0) and (3, 1.5) through mpCamera->project - as one job and
as three jobs in one call (the three pairs).
usage: tests/tools/bench_sim3_search.py [--reps N] [--out profiles/sim3_bench.json]

Per shape: the wall time of the call (median over the repetitions, host clock around the Python wrapper), the library's own timer,
the HIP-event times of the three kernels, and from the restatement the share of the points that enter the walk.  Every result is
compared with the restatement before it is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from tests import sim3_cases as s3  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = orb.Context(0)
case = s3.random_case("pinhole:752x480:2000:3")
_, gF = case["view"]()
M = len(case["valid"])
res = dict(library=orb.version(), device=ctx.device_name, frame=[752, 480], keypoints=int(gF.N), points=M, reps=args.reps,
           held_on_entry=int((case["matched"] != -1).sum()), shapes=[])
FORMS = {(8, 1.5): True, (5, 1.0): False, (3, 1.5): False}


def median_ms(fn, reps):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def stat_ms(name):
    total, calls = ctx.get_stat(name)
    return total / max(calls, 1)


def measure(tag, jobs, refs):
    call = lambda: orb.search_keyframe_sim3(ctx, gF, jobs, want_stage=False)
    g = orb.search_keyframe_sim3(ctx, gF, jobs)
    for k, r in enumerate(refs):
        assert all(np.array_equal(g[k][f], r[f]) for f in ("matched", "point_keypoint", "stage")) and g[k]["n_matches"] == r["n_matches"], (tag, k)
    ctx.set_kernel_timing(False)
    wall, p10, p90 = median_ms(call, args.reps)
    ctx.reset_stats()
    for _ in range(args.reps):
        call()
    own = stat_ms("sim3.total")
    ctx.set_kernel_timing(True)
    ctx.reset_stats()
    for _ in range(args.reps):
        call()
    kern = {k: round(stat_ms("kernel.sim3_" + k), 4) for k in ("grid", "candidates", "resolve")}
    ctx.set_kernel_timing(False)
    shape = dict(shape=tag, jobs=len(jobs), median_wall_ms=round(wall, 4), p10_wall_ms=round(p10, 4), p90_wall_ms=round(p90, 4),
                 library_ms=round(own, 4), kernels_ms=kern,
                 restatement=[dict(n_matches=r["n_matches"], walk=r["stats"]["walk"], walk_share=round(r["stats"]["walk"] / M, 4),
                                   searched=int(r["stats"]["stages"][0] + r["stats"]["stages"][7]), changed_by_locks=r["stats"]["changed_by_locks"],
                                   max_candidates=r["stats"]["max_candidates"]) for r in refs])
    res["shapes"].append(shape)
    print(json.dumps(shape), flush=True)


refs = {p: s3.expected(case, p[0], p[1], hand) for p, hand in FORMS.items()}
for p, hand in FORMS.items():
    measure(f"th{p[0]}_ratio{p[1]}", [s3.job_of(case, p[0], p[1], hand)], [refs[p]])
measure("three_jobs", [s3.job_of(case, p[0], p[1], hand) for p, hand in FORMS.items()], [refs[p] for p in FORMS])
line = json.dumps(res)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
print(line)

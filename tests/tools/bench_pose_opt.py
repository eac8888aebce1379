#!/usr/bin/env python3
"""Latency of ft_pose_optimization on an MI355X (not part of the test suite): batches of 1, 16 and 128 frames at 100, 300 and 1 000
observations per frame (pinhole frames with mono and stereo keypoints, one level sigma of pixel noise, a tenth of the observations
gross outliers, the initial pose 0.02 rad / 0.05 m off: the frames of tests/pose_opt_cases.py).
usage: tests/tools/bench_pose_opt.py [--reps N] [--out profiles/pose_opt_bench.json]

Per shape: wall time of the call through ctypes on argument arrays built once (median [10th, 90th percentile] over the
repetitions, ms), the library's own timer, the HIP-event time of k_pose_opt (a run of its own), and the work the frames did:
evaluations of the edge set with and without the quadratic form, summed over the batch (from the trace).  The restatement on the
same machine is not a baseline and is not timed.  No time is a pass criterion."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import _capi, orb  # noqa: E402
from tests import pose_opt_cases as pc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = orb.Context(0)
res = dict(library=orb.version(), device=ctx.device_name, reps=args.reps, shapes=[])


def pct(ts):
    return [round(float(np.median(ts)), 4), round(float(np.percentile(ts, 10)), 4), round(float(np.percentile(ts, 90)), 4)]


def stat_ms(name):
    total, calls = ctx.get_stat(name)
    return round(total / max(calls, 1), 4)


for n_obs in (100, 300, 1000):
    pool = [pc.to_device(orb, pc.frame("mixed", 200 + s, n_obs, noise=1.0, outliers=0.1)) for s in range(16)]
    for n_frames in (1, 16, 128):
        frames = [pool[f % 16] for f in range(n_frames)]
        F = (_capi.PoseOptFrame * n_frames)(*[f.c for f in frames])
        T = (_capi.SE3 * n_frames)()
        outs = [np.zeros(n_obs, np.uint8) for _ in frames]
        O = (C.c_void_p * n_frames)(*[_capi.ptr(o) for o in outs])
        ret = np.zeros(n_frames, np.int32)
        tr = (_capi.PoseOptTrace * n_frames)()
        L = _capi.lib()

        def call():
            assert L.ft_pose_optimization(ctx._h, n_frames, F, T, O, _capi.ptr(ret), tr) == 0

        call()
        ctx.set_kernel_timing(False)
        ctx.reset_stats()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        own = stat_ms("pose_optimization.total")
        ctx.set_kernel_timing(True)
        ctx.reset_stats()
        for _ in range(args.reps):
            call()
        kernel = stat_ms("kernel.pose_opt")
        ctx.set_kernel_timing(False)
        full = sum(tr[f].iterations[r] for f in range(n_frames) for r in range(4))
        trials = sum(tr[f].iterations[r] + tr[f].rejected[r] for f in range(n_frames) for r in range(4))  # a lower bound: accepted + rejected
        shape = dict(frames=n_frames, observations=n_obs, wall_ms=pct(ts), library_ms=own, kernel_ms=kernel,
                     frames_per_s=round(n_frames / (np.median(ts) * 1e-3)), inliers_mean=round(float(ret.mean()), 1),
                     system_builds=full, trial_evaluations_at_least=trials, launches=ctx.get_stat("pose_optimization.launches")[0] / args.reps)
        res["shapes"].append(shape)
        print(json.dumps(shape), flush=True)
line = json.dumps(res)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
print(line)

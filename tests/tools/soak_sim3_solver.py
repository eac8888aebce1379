#!/usr/bin/env python3
"""Long randomized parity run of ft_sim3_solver on an MI355X (not part of the test suite) against the restatement
(tests/sim3_solver_ref.py).
usage: tests/tools/soak_sim3_solver.py [--trials N] [--seed S] [--out profiles/sim3_solver_soak.json]

A trial draws 1 .. 8 problems: a pairing of camera models (pinhole, KannalaBrandt8), 3 .. 300 pairs among up to three times as many
entries, 10 .. 90 % planted inliers, a free or a fixed scale, a random rotation (0.15 rad per axis, 1 sigma) and translation (0.3 m), min_inliers between 0
and the pair count plus 2 (so that some problems have no job), 1 .. 120 iterations asked for, random draws.  The problems go to the
device in one call.  Every field must equal the restatement's: the integers, the flags and the per-iteration counts exactly, the
floats bit for bit.  Exit code 1 on any mismatch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from tests import sim3_solver_cases as sc  # noqa: E402
from tests import sim3_solver_ref as ref  # noqa: E402

INTS = ("converged", "no_more", "iterations", "effective_iterations", "n_inliers", "n_best_inliers", "best_iteration")
ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=40)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--out", default=None)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
ctx = orb.Context(0)
problems = mismatches = jobless = converged = hypotheses = rejected = 0
models = ("pinhole", "kb8", "kb8b")
t0 = time.time()
for trial in range(args.trials):
    batch = []
    for _ in range(int(rng.integers(1, 9))):
        N = int(rng.integers(3, 301))
        fix = bool(rng.integers(0, 2))
        try:
            batch.append(sc.problem.__wrapped__(int(rng.integers(0, 1 << 30)), N, int(round(N * rng.uniform(0.1, 0.9))), n=N + int(rng.integers(0, 2 * N + 1)),
                                                cams=(models[int(rng.integers(0, 3))], models[int(rng.integers(0, 3))]), fix_scale=fix,
                                                scale=1.0 if fix else float(rng.uniform(0.5, 2.0)), rotvec=tuple(rng.normal(0, 0.15, 3)),
                                                trans=tuple(rng.normal(0, 0.3, 3)), min_inliers=int(rng.integers(0, N + 3)),
                                                max_iterations=int(rng.integers(1, 121))))
        except AssertionError:  # the generator refuses a geometry whose outliers are not gross or whose points come too close: draw another
            rejected += 1
    got = orb.sim3_solver(ctx, [sc.to_device(orb, P) for P in batch])
    for i, (P, g) in enumerate(zip(batch, got)):
        want = ref.sim3_solver(P)
        problems += 1
        jobless += want["effective_iterations"] == 0
        converged += want["converged"]
        hypotheses += want["effective_iterations"]
        bad = [f for f in INTS if g[f] != want[f]]
        bad += [f for f in ("T12", "R", "t", "s") if not np.array_equal(np.ascontiguousarray(g[f], np.float32).view(np.uint32),
                                                                        np.ascontiguousarray(want[f], np.float32).view(np.uint32))]
        bad += [f for f in ("inliers", "best_inliers", "hypothesis_inliers") if not np.array_equal(g[f], want[f])]
        if bad:
            mismatches += 1
            print(f"MISMATCH trial {trial} problem {i}: {int(P['valid'].sum())} pairs, models {P['cam_model1']} {P['cam_model2']}: {bad}")
summary = dict(seed=args.seed, trials=args.trials, problems=problems, jobless=int(jobless), converged=int(converged), hypotheses=int(hypotheses), rejected_geometries=rejected,
               mismatches=mismatches, library=orb.version(), device=ctx.device_name, seconds=round(time.time() - t0, 1))
print(f"sim3-solver soak: {json.dumps(summary)}")
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(summary) + "\n")
sys.exit(1 if mismatches else 0)

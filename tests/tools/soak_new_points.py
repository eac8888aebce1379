#!/usr/bin/env python3
"""Long randomized parity run of the triangulation of LocalMapping::CreateNewMapPoints on an MI355X (not part of the test suite):
ft_triangulate_new_points against the restatement (tests/new_points_ref.py), and ft_search_and_triangulate against the two calls.
usage: tests/tools/soak_new_points.py [--trials N] [--seed S] [--out profiles/new_points_soak.json]

A trial draws a camera form (pinhole with stereo keypoints, KannalaBrandt8 with one or two cameras), 40 .. 700 features, 1 .. 4
neighbours, mbInertial, mbFarPoints with a threshold between 2 m and 200 m and a ratio factor (tests/new_points_cases.py scenario:
true and wrong correspondences, far points, pairs around the chi-square limits, octaves four levels apart).  status, x3d, n_points
and first_neighbour must be equal bit for bit.  Every fourth trial also runs a tests/triangulation_cases.py scenario through
ft_search_and_triangulate and through ft_search_for_triangulation + ft_triangulate_new_points: every output must be equal.  Prints
one line per failure and a summary; exit code 1 on any mismatch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from tests import new_points_cases as nc  # noqa: E402
from tests import new_points_ref as npr  # noqa: E402
from tests import triangulation_cases as tc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=60)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--out", default=None)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
ctx = orb.Context(0)
calls = rows = fused_calls = mismatches = 0
status_counts = {}
t0 = time.time()
for trial in range(args.trials):
    form = nc.FORMS[int(rng.integers(0, 3))]
    n1, nn = int(rng.integers(40, 701)), int(rng.integers(1, 5))
    S = nc.scenario.__wrapped__(form, int(rng.integers(0, 1 << 30)), n1, nn)
    P = dict(inertial=bool(rng.random() < 0.5), far_points=bool(rng.random() < 0.6), th_far=float(rng.choice([2.0, 3.0, 40.0, 200.0])),
             ratio_factor=float(np.float32(1.5) * np.float32(rng.choice([1.1, 1.2, 1.3]))))
    want = npr.triangulate_new_points(S["kf1"], S["g1"], S["neighbours"], S["geometries"], S["matches12"], **P)
    got = orb.triangulate_new_points(ctx, tc.to_device(orb, S["kf1"]), nc.to_device_geometry(orb, S["g1"]), [tc.to_device(orb, k) for k in S["neighbours"]],
                                     [nc.to_device_geometry(orb, g) for g in S["geometries"]], S["matches12"], P["inertial"], P["far_points"],
                                     P["th_far"], P["ratio_factor"])
    calls += 1
    rows += nn
    bad = [f for f in ("status", "n_points", "first_neighbour") if not np.array_equal(got[f], want[f])]
    bad += ["x3d"] if not np.array_equal(got["x3d"].view(np.uint32), want["x3d"].view(np.uint32)) else []
    for v, c in zip(*np.unique(want["status"], return_counts=True)):
        status_counts[int(v)] = status_counts.get(int(v), 0) + int(c)
    if trial % 4 == 0:
        T = tc.scenario.__wrapped__(form, int(rng.integers(0, 1 << 30)), n=int(rng.integers(60, 401)), neighbours=nn, levelsup=int(rng.integers(1, 4)))
        k1, g1 = tc.to_device(orb, T["kf1"]), nc.to_device_geometry(orb, nc.geometry_from_pair(T["kf1"], T["pairs"][0], True))
        k2 = [tc.to_device(orb, k) for k in T["neighbours"]]
        g2 = [nc.to_device_geometry(orb, nc.geometry_from_pair(k, p, False)) for k, p in zip(T["neighbours"], T["pairs"])]
        ps = [tc.to_device_pair(orb, p) for p in T["pairs"]]
        flags = (False, bool(rng.random() < 0.3), bool(rng.random() < 0.7))
        s = orb.search_for_triangulation(ctx, k1, k2, ps, *flags)
        t = orb.triangulate_new_points(ctx, k1, g1, k2, g2, s["matches12"], P["inertial"], P["far_points"], P["th_far"], P["ratio_factor"])
        f = orb.search_and_triangulate(ctx, k1, g1, k2, g2, ps, *flags, inertial=P["inertial"], far_points=P["far_points"],
                                       th_far_points=P["th_far"], ratio_factor=P["ratio_factor"])
        fused_calls += 1
        bad += ["fused " + n for n in ("matches12", "n", "best_dist") if not np.array_equal(f[n], s[n])]
        bad += ["fused " + n for n in ("status", "x3d", "n_points", "first_neighbour") if not np.array_equal(f[n], t[n])]
    if bad:
        mismatches += 1
        print(f"MISMATCH trial {trial} {form} n1 {n1} neighbours {nn} {P}: {bad}")
summary = dict(seed=args.seed, trials=args.trials, standalone_calls=calls, neighbour_rows=rows, fused_calls=fused_calls, mismatches=mismatches,
               status_counts={str(k): status_counts[k] for k in sorted(status_counts)}, library=orb.version(), device=ctx.device_name,
               seconds=round(time.time() - t0, 1))
print(f"new-points soak: {json.dumps(summary)}")
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(summary) + "\n")
sys.exit(1 if mismatches else 0)

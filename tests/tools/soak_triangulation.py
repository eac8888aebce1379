#!/usr/bin/env python3
"""Long randomized parity run of ORBmatcher::SearchForTriangulation on an MI355X (not part of the test suite):
ft_search_for_triangulation against the sequential restatement (tests/triangulation_ref.py).
usage: tests/tools/soak_triangulation.py [--trials N] [--seed S]

A trial draws a camera form (pinhole, KannalaBrandt8 with one or two cameras), 60 .. 500 features, 1 .. 6 neighbours (now and
then an empty one and one without a shared node), sideways or forward motion, the vocabulary level (nodes of a few features up
to ONE node with everything), and bOnlyStereo / bCoarse / mbCheckOrientation (tests/triangulation_cases.py scenario: distractors
off the epipolar line, exact duplicates, distances of 50 and 51, keypoints around the epipole).  matches12, nmatches and bestDist
must be equal, and the batched call must equal the single calls.  Prints one line per failure and a summary; exit code 1 on any
mismatch."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from tests import triangulation_cases as tc  # noqa: E402
from tests import triangulation_ref as tr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=60)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
ctx = orb.Context(0)
calls = pairs = mismatches = 0
tot = dict(matches=0, nearest_rejected=0, next_won=0, epipole_rejections=0, ties=0, removed_by_histogram=0)
t0 = time.time()
for trial in range(args.trials):
    form = tc.FORMS[int(rng.integers(0, 3))]
    kw = dict(n=int(rng.integers(60, 501)), neighbours=int(rng.integers(1, 5)), forward=bool(rng.random() < 0.4),
              levelsup=int(rng.integers(1, 4)), empty_neighbour=bool(rng.random() < 0.2), foreign_neighbour=bool(rng.random() < 0.2))
    if kw["neighbours"] == 1:
        kw["empty_neighbour"] = False  # (it is inserted behind the first neighbour)
    flags = (bool(rng.random() < 0.25), bool(rng.random() < 0.3), bool(rng.random() < 0.7))
    S = tc.scenario.__wrapped__(form, int(rng.integers(0, 1 << 30)), **kw)
    kf1 = tc.to_device(orb, S["kf1"])
    k2 = [tc.to_device(orb, k) for k in S["neighbours"]]
    ps = [tc.to_device_pair(orb, p) for p in S["pairs"]]
    g = orb.search_for_triangulation(ctx, kf1, k2, ps, *flags)
    calls += 1
    for k, (kf2, p) in enumerate(zip(S["neighbours"], S["pairs"])):
        r = tr.search_for_triangulation(S["kf1"], kf2, p, *flags)
        s = orb.search_for_triangulation(ctx, kf1, [k2[k]], [ps[k]], *flags)
        pairs += 1
        bad = [f for f in ("matches12", "best_dist") if not np.array_equal(g[f][k], r[f])]
        bad += ["n"] if int(g["n"][k]) != r["n"] else []
        bad += ["single != batched"] if not (np.array_equal(s["matches12"][0], g["matches12"][k]) and s["n"][0] == g["n"][k]) else []
        if bad:
            mismatches += 1
            print(f"MISMATCH trial {trial} {form} {kw} {flags} neighbour {k}: {bad}")
        tot["matches"] += r["n"]
        for f in tot:
            if f != "matches":
                tot[f] += r["stats"][f]
print(f"triangulation soak: seed {args.seed}, {calls} batched calls, {pairs} keyframe pairs, {mismatches} mismatches; the restatement saw "
      f"{tot['matches']} matches, {tot['nearest_rejected']} nearest candidates rejected by the constraint ({tot['next_won']} times the next one "
      f"won), {tot['epipole_rejections']} epipole rejections, {tot['ties']} ties, {tot['removed_by_histogram']} histogram removals; "
      f"{orb.version()} on {ctx.device_name}, {time.time() - t0:.0f} s")
sys.exit(1 if mismatches else 0)

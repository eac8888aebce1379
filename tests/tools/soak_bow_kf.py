#!/usr/bin/env python3
"""Long randomized parity run of ORBmatcher::SearchByBoW(KeyFrame, KeyFrame) on an MI355X (not part of the test suite):
ft_search_by_bow_keyframes against the sequential restatement (tests/bow_kf_ref.py).
usage: tests/tools/soak_bow_kf.py [--trials N] [--seed S]

A trial draws one or two cameras, 30 .. 900 features per keyframe, 1 .. 6 neighbours (now and then an empty one, one without map
points and one without a shared node), the vocabulary level (nodes of a few features up to ONE node with everything, which takes
the path of the lists too long for the registers), the share of features with a map point, nn_ratio and mbCheckOrientation
(tests/bow_kf_cases.py scenario: copies at 0 - 14 bits, descriptors around TH_LOW, exact duplicates, one dominant rotation with
outliers); every fourth trial is a single node of a drawn size.  matches12 and nmatches must be equal, and the batched call must
equal the single calls.  Prints one line per failure and a summary; exit code 1 on any mismatch."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from tests import bow_kf_cases as bc  # noqa: E402
from tests import bow_kf_ref as br  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=60)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
ctx = orb.Context(0)
calls = pairs = mismatches = 0
tot = dict(matches=0, dist_50=0, ratio_rejections=0, claims_changed_a_choice=0, removed_by_histogram=0, skipped_by_n_un=0)
longest = 0
t0 = time.time()
for trial in range(args.trials):
    cfg = (float(rng.choice([0.6, 0.7, 0.75, 0.9, 1.0, 1.5])), bool(rng.random() < 0.7))
    if trial % 4 == 3:
        kw = dict(k1=int(rng.integers(1, 200)), k2=int(rng.choice([1, 15, 16, 17, 63, 64, 65, 255, 256, 257, int(rng.integers(1, 900))])),
                  seed=int(rng.integers(0, 1 << 20)), extra1=int(rng.integers(0, 10)), extra2=int(rng.integers(0, 40)))
        S = bc.node_size_case.__wrapped__(**kw)
    else:
        nn = int(rng.integers(1, 5))
        kw = dict(n1=int(rng.integers(30, 901)), n2=tuple(int(v) for v in rng.integers(30, 901, nn)), levelsup=int(rng.integers(1, 5)),
                  two_cam=bool(rng.random() < 0.4), empty_neighbour=bool(nn > 1 and rng.random() < 0.2),
                  pointless_neighbour=bool(rng.random() < 0.2), foreign_neighbour=bool(rng.random() < 0.2),
                  has1=float(rng.uniform(0.3, 1.0)), has2=float(rng.uniform(0.3, 1.0)))
        S = bc.scenario.__wrapped__(int(rng.integers(0, 1 << 30)), **kw)
    kf1 = bc.to_device(orb, S["kf1"])
    k2 = [bc.to_device(orb, k) for k in S["neighbours"]]
    g = orb.search_by_bow_keyframes(ctx, kf1, k2, *cfg)
    calls += 1
    for k, nb in enumerate(S["neighbours"]):
        r = br.search_by_bow_keyframes(S["kf1"], nb, *cfg)
        s = orb.search_by_bow_keyframes(ctx, kf1, [k2[k]], *cfg)
        pairs += 1
        bad = ["matches12"] if not np.array_equal(g["matches12"][k], r["matches12"]) else []
        bad += ["n"] if int(g["n"][k]) != r["n"] else []
        bad += ["single != batched"] if not (np.array_equal(s["matches12"][0], g["matches12"][k]) and s["n"][0] == g["n"][k]) else []
        if bad:
            mismatches += 1
            print(f"MISMATCH trial {trial} {kw} {cfg} neighbour {k}: {bad}")
        tot["matches"] += r["n"]
        for f in tot:
            if f != "matches":
                tot[f] += r["stats"][f]
        longest = max([longest] + [b for _, b in r["stats"]["node_sizes"]])
print(f"keyframe BoW soak: seed {args.seed}, {calls} batched calls, {pairs} keyframe pairs, {mismatches} mismatches; the restatement saw "
      f"{tot['matches']} matches, {tot['dist_50']} best distances of exactly 50, {tot['ratio_rejections']} ratio rejections, "
      f"{tot['claims_changed_a_choice']} choices changed by a claim, {tot['removed_by_histogram']} histogram removals, "
      f"{tot['skipped_by_n_un']} features beyond n_un, longest candidate list {longest}; {orb.version()} on {ctx.device_name}, "
      f"{time.time() - t0:.0f} s")
sys.exit(1 if mismatches else 0)

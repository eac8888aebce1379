#!/usr/bin/env python3
"""Randomised parity run of ORBmatcher::SearchByBoW(KeyFrame, Frame) over the candidates of a relocalisation on an MI355X (not
part of the test suite): ft_search_by_bow_candidates against the oracle's per-candidate results.
usage: tests/tools/soak_bow_reloc.py [--trials N] [--seed S] [--out FILE]

A trial draws one or two cameras, 30 .. 900 features for the frame and per candidate, 1 .. 6 candidates (now and then an empty
one, one without map points and one without a shared node), the vocabulary level (nodes of a few features up to ONE node with
everything, which takes the path of the frame nodes too long for the registers), the share of features with a map point, nn_ratio
and mbCheckOrientation (tests/bow_reloc_cases.py scenario); every fourth trial is a single node of drawn sizes.  Rows and counts
must be equal, and the batched call must equal ft_search_by_bow per candidate.  Prints one line per failure and a summary; exit
code 1 on any mismatch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from tests import bow_reloc_cases as rc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=60)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--out", default=None)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
ctx = orb.Context(0)
calls = pairs = mismatches = matches = right = longest = 0
t0 = time.time()
for trial in range(args.trials):
    cfg = (float(rng.choice([0.6, 0.7, 0.75, 0.9, 1.0, 1.5])), bool(rng.random() < 0.7))
    if trial % 4 == 3:
        kw = dict(k_kf=int(rng.integers(1, 200)), k_f=int(rng.choice([1, 15, 16, 17, 63, 64, 65, 255, 256, 257, int(rng.integers(1, 900))])),
                  two_cam=bool(rng.random() < 0.4), seed=int(rng.integers(0, 1 << 20)))
        S = rc.node_size_case.__wrapped__(**kw)
    else:
        nk = int(rng.integers(1, 5))
        kw = dict(n_f=int(rng.integers(30, 901)), n_k=tuple(int(v) for v in rng.integers(30, 901, nk)), levelsup=int(rng.integers(1, 5)),
                  two_cam=bool(rng.random() < 0.4), empty_candidate=bool(nk > 1 and rng.random() < 0.2),
                  pointless_candidate=bool(rng.random() < 0.2), foreign_candidate=bool(rng.random() < 0.2), has=float(rng.uniform(0.3, 1.0)))
        S = rc.scenario.__wrapped__(int(rng.integers(0, 1 << 30)), **kw)
    frame, ks = rc.to_device(orb, S)
    g = orb.search_by_bow_candidates(ctx, frame, ks, S["nleft"], *cfg)
    want = rc.oracle(S, *cfg)
    calls += 1
    longest = max(longest, int(np.diff(S["frame"]["fv_offsets"]).max(initial=0)))
    for k, c in enumerate(S["candidates"]):
        s = orb.search_by_bow(ctx, ks[k].side, c["has_point"], frame, S["nleft"], *cfg)
        pairs += 1
        bad = ["matches"] if not np.array_equal(g["matches"][k], want[k]["matches"]) else []
        bad += ["n"] if int(g["n"][k]) != want[k]["n"] else []
        bad += ["single != batched"] if not (np.array_equal(s["matches"], g["matches"][k]) and s["n"] == g["n"][k]) else []
        if bad:
            mismatches += 1
            print(f"MISMATCH trial {trial} {kw} {cfg} candidate {k}: {bad}")
        matches += want[k]["n"]
        if S["nleft"] != -1:
            right += int((want[k]["matches"][S["nleft"]:] >= 0).sum())
summary = dict(library=orb.version(), device=ctx.device_name, seed=args.seed, trials=args.trials, batched_calls=calls, candidate_rows=pairs,
               mismatches=mismatches, oracle_matches=matches, right_camera_matches=right, longest_frame_node=longest,
               seconds=round(time.time() - t0, 1))
print(json.dumps(summary))
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(summary) + "\n")
sys.exit(1 if mismatches else 0)

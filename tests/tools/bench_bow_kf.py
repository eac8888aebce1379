#!/usr/bin/env python3
"""Latency of ft_search_by_bow_keyframes on an MI355X (not part of the test suite): keyframes of 2 000 features, about half of them
holding a map point, FeatureVectors from a k = 10, L = 5 tree at levelsup 3 (about 100 nodes), 1, 6, 18 and 36 neighbours.
usage: tests/tools/bench_bow_kf.py [--reps N] [--out profiles/bow_kf_bench.json]

Per neighbour count: the wall time of the batched call (host clock around the call, which ends in its stream synchronise: median,
10th and 90th percentile over the repetitions) and, as the comparison, the same neighbours as single-neighbour calls of the same
entry point - the two are timed alternately, repetition by repetition.  Then, in runs of their own, the library's own timer and
the HIP-event times of the two kernels.  For orientation only, ft_search_by_bow on one of the pairs: a different function
(KeyFrame against Frame), not a baseline.  The neighbours of a call cycle through six distinct keyframes.  Before anything is
timed the batched result is compared with the restatement (tests/bow_kf_ref.py), whose stats give the node-size distribution."""
import argparse
import json
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
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--features", type=int, default=2000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = orb.Context(0)
N = args.features
S = bc.scenario.__wrapped__(9, n1=N, n2=(N,) * 6, levelsup=3, vocab=(10, 5, 3), has1=0.5, has2=0.5)
kf1 = bc.to_device(orb, S["kf1"])
k6 = [bc.to_device(orb, k) for k in S["neighbours"]]

want = [br.search_by_bow_keyframes(S["kf1"], nb) for nb in S["neighbours"]]
got = orb.search_by_bow_keyframes(ctx, kf1, k6)
assert all(np.array_equal(got["matches12"][k], w["matches12"]) and got["n"][k] == w["n"] for k, w in enumerate(want)), "differs from the restatement"
lists2 = np.array([b for w in want for _, b in w["stats"]["node_sizes"]])
lists1 = np.array([a for w in want for a, _ in w["stats"]["node_sizes"]])
el2 = np.array([v for w in want for v in w["stats"]["eligible2"]])
el1 = np.array([v for w in want for v in w["stats"]["eligible1"]])


def dist(a):
    return dict(units=int(len(a)), median=float(np.median(a)), p90=float(np.percentile(a, 90)), p99=float(np.percentile(a, 99)), max=int(a.max()),
                share_le_16=round(float((a <= 16).mean()), 4), share_le_64=round(float((a <= 64).mean()), 4))


res = dict(library=orb.version(), device=ctx.device_name, features=N, vocabulary="k 10, L 5, levelsup 3", reps=args.reps,
           has_point_share=0.5, shared_nodes_per_pair=float(np.mean([w["stats"]["shared_nodes"] for w in want])),
           matches_per_pair=float(np.mean([w["n"] for w in want])),
           node_sizes=dict(list_keyframe1=dist(lists1), list_keyframe2=dist(lists2), eligible_keyframe1=dist(el1), eligible_candidates=dist(el2)),
           shapes=[])


def stat_ms(name):
    total, calls = ctx.get_stat(name)
    return total / max(calls, 1)


def spread(ts):
    return dict(median=round(float(np.median(ts)), 4), p10=round(float(np.percentile(ts, 10)), 4), p90=round(float(np.percentile(ts, 90)), 4))


def clock(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


for nn in (1, 6, 18, 36):
    k2 = [k6[i % 6] for i in range(nn)]
    batched = lambda: orb.search_by_bow_keyframes(ctx, kf1, k2)
    singles = lambda: [orb.search_by_bow_keyframes(ctx, kf1, [k]) for k in k2]
    ctx.set_kernel_timing(False)
    for _ in range(3):
        batched(), singles()
    tb, ts = [], []
    for _ in range(args.reps):  # alternately: what else runs on the host hits both alike
        tb.append(clock(batched))
        ts.append(clock(singles))
    ctx.reset_stats()
    for _ in range(args.reps):
        batched()
    own = stat_ms("search_by_bow_keyframes.total")
    ctx.set_kernel_timing(True)
    ctx.reset_stats()
    for _ in range(args.reps):
        batched()
    km, kf = stat_ms("kernel.bow_kf_match"), stat_ms("kernel.bow_kf_finish")
    ctx.set_kernel_timing(False)
    res["shapes"].append(dict(neighbours=nn, batched_wall_ms=spread(tb), batched_library_ms=round(own, 4), kernel_bow_kf_match_ms=round(km, 4),
                              kernel_bow_kf_finish_ms=round(kf, 4), single_calls_wall_ms=spread(ts),
                              launches_batched=2, launches_single_calls=2 * nn, copies_batched=2, copies_single_calls=2 * nn))
    print(json.dumps(res["shapes"][-1]), flush=True)
# for orientation: the KeyFrame, Frame overload on one of the pairs (another function: no n_un test, <= TH_LOW, the frame's claims)
a, b = S["kf1"], S["neighbours"][0]
side = lambda k: orb.BowSide(k["fv_nodes"], k["fv_offsets"], k["fv_features"], k["descriptors"], k["angles"])
sa, sb = side(a), side(b)
other = lambda: orb.search_by_bow(ctx, sa, a["has_point"], sb)
for _ in range(3):
    other()
res["search_by_bow_one_pair_wall_ms"] = spread([clock(other) for _ in range(args.reps)])
line = json.dumps(res)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
print(line)

#!/usr/bin/env python3
"""Latency of ft_search_by_bow_candidates on an MI355X (not part of the test suite): a frame and candidate keyframes of 2 000
features, half of the candidates' features holding a map point, FeatureVectors from a k = 10, L = 5 tree at levelsup 3 (about 100
nodes), 1, 5, 15 and 40 candidates.
usage: tests/tools/bench_bow_reloc.py [--reps N] [--out profiles/bow_reloc_bench.json]

Per candidate count: the wall time of the batched call (host clock around the call, which ends in its stream synchronise: median,
10th and 90th percentile over the repetitions) and, as the baseline, the same candidates as N calls of ft_search_by_bow - the loop
of Tracking::Relocalization as the library served it before; the two are timed alternately, repetition by repetition.  Then, in
runs of their own, the library's own timer and the HIP-event times of the two kernels.  The candidates of a call cycle through six
distinct keyframes.  Before anything is timed the batched result is compared with the oracle's per-candidate results."""
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
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--features", type=int, default=2000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = orb.Context(0)
N = args.features
S = rc.scenario.__wrapped__(9, n_f=N, n_k=(N,) * 6, levelsup=3, vocab=(10, 5, 3), has=0.5)
frame, k6 = rc.to_device(orb, S)
has6 = [c["has_point"] for c in S["candidates"]]

want = rc.oracle(S)
got = orb.search_by_bow_candidates(ctx, frame, k6)
assert all(np.array_equal(got["matches"][k], w["matches"]) and got["n"][k] == w["n"] for k, w in enumerate(want)), "differs from the oracle"
sizes_f = np.diff(S["frame"]["fv_offsets"])
sizes_k = np.concatenate([np.diff(c["fv_offsets"]) for c in S["candidates"]])


def dist(a):
    return dict(lists=int(len(a)), median=float(np.median(a)), p90=float(np.percentile(a, 90)), max=int(a.max()))


res = dict(library=orb.version(), device=ctx.device_name, features=N, vocabulary="k 10, L 5, levelsup 3", reps=args.reps,
           has_point_share=0.5, matches_per_candidate=float(np.mean([w["n"] for w in want])),
           node_sizes=dict(frame=dist(sizes_f), candidates=dist(sizes_k)), shapes=[])


def stat_ms(name):
    total, calls = ctx.get_stat(name)
    return total / max(calls, 1)


def spread(ts):
    return dict(median=round(float(np.median(ts)), 4), p10=round(float(np.percentile(ts, 10)), 4), p90=round(float(np.percentile(ts, 90)), 4))


def clock(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


for nk in (1, 5, 15, 40):
    ks = [k6[i % 6] for i in range(nk)]
    hs = [has6[i % 6] for i in range(nk)]
    batched = lambda: orb.search_by_bow_candidates(ctx, frame, ks)
    singles = lambda: [orb.search_by_bow(ctx, k.side, h, frame, -1, 0.75, True) for k, h in zip(ks, hs)]
    b, s = batched(), singles()
    assert all(np.array_equal(b["matches"][k], s[k]["matches"]) and b["n"][k] == s[k]["n"] for k in range(nk)), "batched != single calls"
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
    own = stat_ms("search_by_bow_candidates.total")
    ctx.set_kernel_timing(True)
    ctx.reset_stats()
    for _ in range(args.reps):
        batched()
    km, kf = stat_ms("kernel.bow_cand_match"), stat_ms("kernel.bow_cand_finish")
    ctx.set_kernel_timing(False)
    res["shapes"].append(dict(candidates=nk, batched_wall_ms=spread(tb), batched_library_ms=round(own, 4), kernel_bow_cand_match_ms=round(km, 4),
                              kernel_bow_cand_finish_ms=round(kf, 4), single_calls_wall_ms=spread(ts),
                              launches_batched=2, launches_single_calls=nk, copies_batched=2, copies_single_calls=2 * nk))
    print(json.dumps(res["shapes"][-1]), flush=True)
line = json.dumps(res)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
print(line)

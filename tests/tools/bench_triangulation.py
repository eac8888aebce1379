#!/usr/bin/env python3
"""Latency of ft_search_for_triangulation on an MI355X (not part of the test suite): keyframes of 2 000 features, FeatureVectors
from a k = 10, L = 5 tree at levelsup 4, 10 and 30 neighbours, pinhole and KannalaBrandt8 with two cameras.
usage: tests/tools/bench_triangulation.py [--reps N] [--out profiles/triangulation_bench.json]

Per shape: the wall time of the batched call (median over the repetitions) and the library's own timer, the HIP-event times of the
two kernels, what the same neighbours cost as single calls, and for scale ft_search_by_bow - the nearest existing call - on
the same keyframes, once per neighbour.  The neighbours of a call cycle through five distinct keyframes."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from tests import triangulation_cases as tc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--features", type=int, default=2000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = orb.Context(0)
res = dict(library=orb.version(), device=ctx.device_name, features=args.features, vocabulary="k 10, L 5, levelsup 4", reps=args.reps, shapes=[])


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def stat_ms(name):
    total, calls = ctx.get_stat(name)
    return total / max(calls, 1)


for form in ("pinhole", "kb8x2"):
    S = tc.scenario.__wrapped__(form, 5, n=args.features, neighbours=5, levelsup=4, vocab=(10, 5, 3))
    kf1 = tc.to_device(orb, S["kf1"])
    k5 = [tc.to_device(orb, k) for k in S["neighbours"]]
    p5 = [tc.to_device_pair(orb, p) for p in S["pairs"]]
    bow1 = orb.BowSide(S["kf1"]["fv_nodes"], S["kf1"]["fv_offsets"], S["kf1"]["fv_features"], S["kf1"]["descriptors"], S["kf1"]["keys"]["angle"])
    bow5 = [orb.BowSide(k["fv_nodes"], k["fv_offsets"], k["fv_features"], k["descriptors"], k["keys"]["angle"]) for k in S["neighbours"]]
    has1 = np.ones(len(S["kf1"]["keys"]), np.uint8)
    for nn in (10, 30):
        k2, ps = [k5[i % 5] for i in range(nn)], [p5[i % 5] for i in range(nn)]
        batched = lambda: orb.search_for_triangulation(ctx, kf1, k2, ps)
        g = batched()
        ctx.set_kernel_timing(False)
        wall = median_ms(batched, args.reps)
        ctx.reset_stats()
        for _ in range(args.reps):
            batched()
        own = stat_ms("search_for_triangulation.total")
        ctx.set_kernel_timing(True)
        ctx.reset_stats()
        for _ in range(args.reps):
            batched()
        km, kf = stat_ms("kernel.triang_match"), stat_ms("kernel.triang_finish")
        ctx.set_kernel_timing(False)
        singles = median_ms(lambda: [orb.search_for_triangulation(ctx, kf1, [k2[i]], [ps[i]]) for i in range(nn)], max(args.reps // 3, 3))
        bow = median_ms(lambda: [orb.search_by_bow(ctx, bow1, has1, bow5[i % 5]) for i in range(nn)], max(args.reps // 3, 3))
        sizes = np.diff(S["neighbours"][0]["fv_offsets"])
        res["shapes"].append(dict(form=form, neighbours=nn, features_kf1=len(S["kf1"]["keys"]),
                                  features_neighbour=int(np.mean([len(k["keys"]) for k in S["neighbours"]])), nodes=int(len(sizes)),
                                  node_size_median=float(np.median(sizes)), node_size_max=int(sizes.max()), matches=int(g["n"].sum()),
                                  batched_wall_ms=round(wall, 4), batched_library_ms=round(own, 4), kernel_triang_match_ms=round(km, 4),
                                  kernel_triang_finish_ms=round(kf, 4), single_calls_wall_ms=round(singles, 4),
                                  search_by_bow_calls_wall_ms=round(bow, 4)))
        print(json.dumps(res["shapes"][-1]), flush=True)
line = json.dumps(res)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
print(line)

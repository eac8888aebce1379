#!/usr/bin/env python3
"""Latency of ft_fuse_search on an MI355X (not part of the test suite): keyframes of 2 000 features, 1 500 map points, 1, 10 and
30 targets, a rectified pinhole keyframe (752 x 480, with mvuRight) and a two-camera KannalaBrandt8 keyframe (512 x 512, targets
alternate between the left and the right camera as LocalMapping::SearchInNeighbors calls them).
usage: tests/tools/bench_fuse.py [--reps N] [--out profiles/fuse_bench.json]

Per shape: the wall time of the batched call (median over the repetitions) and the library's own timer, the HIP-event times of
the two kernels, and what the same targets cost as one-target calls (their sum is the batched call's baseline: there is no
earlier implementation).  Every target has a pose of its own (random steps of a few centimetres and degrees), th 3, the
chi-square test on."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from oracle import binding as ob  # noqa: E402
from tests import fuse_cases as fc  # noqa: E402
from tests import reloc_cases as rc  # noqa: E402
from tests import reloc_search_ref as rref  # noqa: E402
from tests import scenarios as sc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--features", type=int, default=2000)
ap.add_argument("--points", type=int, default=1500)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = orb.Context(0)
res = dict(library=orb.version(), device=ctx.device_name, features=args.features, points=args.points, th=3.0, reps=args.reps, shapes=[])


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
    if form == "pinhole":
        w, h = 752, 480
        fr = sc.geometry_frame(w, h, args.features, 21)
        kf, (q, t) = rc.keyframe_points(fr["kL"], fr["dL"], fr["sf"], fr["intr"], w, h, 21)
        _, gF = sc.geometry_views(fr, sc.frame_bounds(w, h))
    else:
        w = h = 512
        fr = sc.geometry_frame(w, h, args.features, 12, two_cameras=True)
        kf, (q, t) = rc.keyframe_points(fr["kL"], fr["dL"], fr["sf"], fr["kb8_intr"], w, h, 12, kb8_cam=sc.KB8_CAM)
        _, gF = sc.geometry_views(fr, sc.frame_bounds(w, h))
    rng = np.random.default_rng(3)
    keep = np.sort(rng.choice(len(kf["valid"]), min(args.points, len(kf["valid"])), replace=False))
    kf = {k: np.asarray(v)[keep] for k, v in kf.items()}
    pts, valid, _ = fc.fuse_points(kf, ob.SE3(q, t), 5)
    poses = [ob.SE3(q, t)] + [ob.SE3(*sc.random_se3(rng)) for _ in range(29)]
    all_targets = [dict(kf=gF, Tcw=orb.SE3(T.q, T.t), Ow=rref.camera_centre(T), log_scale_factor=fr["log_sf"], th=3.0,
                        right=(form == "kb8x2" and k % 2 == 1), cam2=list(sc.KB8_CAM), valid=valid, check_reprojection=True)
                   for k, T in enumerate(poses)]
    for nt in (1, 10, 30):
        tg = all_targets[:nt]
        batched = lambda: orb.fuse_search(ctx, pts, tg)
        g = batched()
        ctx.set_kernel_timing(False)
        wall = median_ms(batched, args.reps)
        ctx.reset_stats()
        for _ in range(args.reps):
            batched()
        own = stat_ms("fuse.total")
        ctx.set_kernel_timing(True)
        ctx.reset_stats()
        for _ in range(args.reps):
            batched()
        kg, ks = stat_ms("kernel.fuse_grid"), stat_ms("kernel.fuse_search")
        ctx.set_kernel_timing(False)
        singles = median_ms(lambda: [orb.fuse_search(ctx, pts, [x]) for x in tg], max(args.reps // 3, 3))
        res["shapes"].append(dict(form=form, targets=nt, keypoints=int(gF.N), points=len(valid), searched=int((g["stage"] == 0).sum()),
                                  found=int(g["n_found"].sum()), batched_wall_ms=round(wall, 4), batched_library_ms=round(own, 4),
                                  kernel_fuse_grid_ms=round(kg, 4), kernel_fuse_search_ms=round(ks, 4), single_calls_wall_ms=round(singles, 4),
                                  singles_over_batched=round(singles / wall, 2)))
        print(json.dumps(res["shapes"][-1]), flush=True)
line = json.dumps(res)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
print(line)

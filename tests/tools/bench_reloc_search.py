"""Latency of ORBmatcher::SearchByProjection(Frame, KeyFrame, sAlreadyFound, th, ORBdist) on one MI355X: the resident call
(ft_tracked_frame_search_keyframe_projection) on a 752x480 frame extracted with nFeatures 2000, with the two parameter sets of
Tracking::Relocalization (th 10 / ORBdist 100 and th 3 / ORBdist 64) on the keyframe points of tests/reloc_cases.py (two per
keypoint, 20 % of the keypoints held on entry).  Beside it, measured in the same run on the same frame: the non-resident entry, and
ft_tracked_frame_search_last_frame_se3 (the closest existing search: same grid, same keypoints, claims resolved in parallel
passes) over the same points at th 15 and th 7.  Every call is timed on its own by the host clock (the calls end in a stream
synchronisation), on a frame uploaded afresh outside the timed window; medians over `reps` calls after a warm-up, and the mean of
the library's own per-call timer (inside the C entry point, without the Python marshalling).
usage: python tests/tools/bench_reloc_search.py [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from fasttrack_amd import orb
from tests import reloc_cases as rc

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
case = rc.random_case("pinhole:752x480:2000:3")
kf, T, log_sf = case["kf"], orb.SE3(case["Tcw"].q, case["Tcw"].t), case["log_sf"]
N, M = len(case["fr"]["kL"]), len(kf["valid"])
ctx = orb.Context(0)
cur = orb.TrackedFrame(ctx, N, max(M, 4096))
view = lambda: case["view"](uright=True)[1]
expect = {p: rc.expected(case, *p) for p in ((10, 100), (3, 64))}
for (th, od), r in expect.items():
    cur.upload(view())
    t = cur.search_keyframe_projection(kf, T, log_sf, th, od)
    assert t["n"] == r["n"] and np.array_equal(t["assign"], r["assign"]) and np.array_equal(cur.holder_obs(), r["holder_obs"])
# the yardstick's points: the same world points, descriptors and observations; octave = the level the relocalisation search predicts
last = dict(valid=kf["valid"], world_pos=kf["world_pos"], descriptors=kf["descriptors"], observations=kf["observations"],
            octave=np.maximum(expect[(10, 100)]["level"], 0), angle=kf["angle"])


def timed(fn, stat, n, prepare):
    """-> (median wall ms of fn alone, mean ms inside the library)"""
    for _ in range(10):
        prepare()
        fn()
    ctx.reset_stats()
    ts = []
    for _ in range(n):
        prepare()
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ms, calls = ctx.get_stat(stat)
    return dict(median_wall_ms=1e3 * float(np.median(ts)), p10_wall_ms=1e3 * float(np.percentile(ts, 10)),
                p90_wall_ms=1e3 * float(np.percentile(ts, 90)), mean_inside_ms=ms / max(calls, 1), calls=int(calls))


def kernels_ms(fn, names, n, prepare):
    ctx.set_kernel_timing(True)
    prepare()
    fn()
    ctx.reset_stats()
    for _ in range(n):
        prepare()
        fn()
    out = {name: ctx.get_stat(name)[0] / max(ctx.get_stat(name)[1], 1) for name in names}
    ctx.set_kernel_timing(False)
    return out


fresh = lambda: cur.upload(view())   # holder_obs back to the state on entry, as for a new frame
gviews = []


def fresh_view():
    gviews[:] = [view()]


out = {"frame": [752, 480], "keypoints": N, "keyframe_points": M, "held_on_entry": int((case["holder"] != -1).sum()), "reps": reps,
       "restatement": {f"th{th}_orb{od}": dict(n=r["n"], **{k: (sorted(v) if isinstance(v, set) else v) for k, v in r["stats"].items()})
                       for (th, od), r in expect.items()}}
for th, od in ((10, 100), (3, 64)):
    tag = f"th{th}_orb{od}"
    out[f"tracked_frame_search_keyframe_projection_{tag}"] = timed(
        lambda: cur.search_keyframe_projection(kf, T, log_sf, th, od), "tracked.search_keyframe_projection.total", reps, fresh)
    out[f"kernels_ms_{tag}"] = kernels_ms(lambda: cur.search_keyframe_projection(kf, T, log_sf, th, od),
                                          ["kernel.reloc_project", "kernel.reloc_candidates", "kernel.reloc_resolve"], reps, fresh)
out["search_keyframe_projection_th10_orb100 (non-resident)"] = timed(
    lambda: orb.KernelController.search_keyframe_projection(ctx, gviews[0], kf, T, log_sf, 10, 100), "search_keyframe_projection.total", reps,
    fresh_view)
for th in (15.0, 7.0):
    out[f"tracked_frame_search_last_frame_se3_th{int(th)} (yardstick)"] = timed(
        lambda: cur.search_last_frame(last, T, th), "tracked.search_last_frame.total", reps, fresh)
out["version"] = orb.version()
print(json.dumps(out))

"""Latency of ORBmatcher::SearchForInitialization on one MI355X: the resident call (ft_tracked_frame_search_for_initialization)
on a 752x480 pair extracted with 5 x 1000 features and the mono lapping area, window 100 - the call
Tracking::MonocularInitialization makes per frame.  Beside it, measured in the same run: ft_tracked_frame_search_last_frame on
the same current frame (the closest existing search: same grid, same N, first-come resolution), and the non-resident entry.
usage: python tests/tools/bench_init_search.py [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from fasttrack_amd import orb, synth
from oracle import binding as ob
from tests import init_search_ref as ref
from tests import scenarios as sc

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
w, h, nf, seed, dx, dy = 752, 480, 5000, 3, 4, 12
sf, _ = ob.scale_factors(1.2, 8)
base = synth.make_image(w, h, seed)
moved = np.roll(base, (dy, dx), axis=(0, 1)).astype(np.int32) + np.random.default_rng(1000 + seed).integers(-3, 4, base.shape)
moved = np.ascontiguousarray(np.clip(moved, 0, 255).astype(np.uint8))
k1, d1, _ = ob.Extractor(nf).extract(base, (0, 1000))
k2, d2, _ = ob.Extractor(nf).extract(moved, (0, 1000))
bounds = sc.frame_bounds(w, h)
intr = synth.intrinsics(w, h)
ctx = orb.Context(0)
g1 = orb.FrameView(k1, d1, sf, bounds)
g2 = orb.FrameView(k2, d2, sf, bounds, mbf=intr["mbf"], mb=intr["mb"], cam=[intr[k] for k in ("fx", "fy", "cx", "cy")])
ini, cur = orb.TrackedFrame(ctx, len(k1), 1), orb.TrackedFrame(ctx, len(k2), 4096)
ini.upload(g1)
cur.upload(g2)
prev = np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32)
o = ref.search_for_initialization(k1, d1, ob.FrameView(k2, d2, sf, bounds), prev)
t = cur.search_for_initialization(ini, prev)
assert t["n"] == o["n"] and np.array_equal(t["matches12"], o["matches12"])
# the yardstick: the motion-model search over as many last-frame points as the initial frame has level-0 keypoints
depth = np.full(len(k2), 4.0, np.float32)
last, Tcw = sc.last_frame_scenario(k2, d2, np.full(len(k2), -1.0, np.float32), depth, intr, w, h, seed=4)


def library_ms(fn, name, n):
    """median-free mean of the library's own per-call timer (inside the C entry point, without the Python marshalling)"""
    for _ in range(5):
        fn()
    ctx.reset_stats()
    for _ in range(n):
        fn()
    ms, calls = ctx.get_stat(name)
    return ms / max(calls, 1)


def wall_ms(fn, n):
    fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def kernels_ms(fn, names, n):
    ctx.set_kernel_timing(True)
    fn()
    ctx.reset_stats()
    for _ in range(n):
        fn()
    out = {}
    for name in names:
        ms, calls = ctx.get_stat(name)
        out[name] = ms / max(calls, 1)
    ctx.set_kernel_timing(False)
    return out


def run_init():
    return cur.search_for_initialization(ini, prev)


def run_last():
    cur.upload(g2)  # (holder_obs back to -1, as for a new frame)
    return cur.search_last_frame(last, Tcw, 15.0)


out = {"frame": [w, h], "N1": int(len(k1)), "N2": int(len(k2)), "level0_F1": int((k1["octave"] == 0).sum()),
       "level0_F2": int((k2["octave"] == 0).sum()), "candidates": o["stats"]["candidates"], "n_matches": o["n"],
       "last_frame_points": int(len(last["valid"])),
       "inside_the_library_ms": {
           "tracked_frame_search_for_initialization": library_ms(run_init, "tracked.search_for_initialization.total", reps),
           "search_for_initialization (non-resident)": library_ms(
               lambda: orb.KernelController.search_for_initialization(ctx, g1, g2, prev), "search_for_initialization.total", reps),
           "tracked_frame_search_last_frame (yardstick)": library_ms(run_last, "tracked.search_last_frame.total", reps)},
       "wall_ms_with_python": {"tracked_frame_search_for_initialization": wall_ms(run_init, reps)},
       "kernels_ms": kernels_ms(run_init, ["kernel.init_prepare", "kernel.init_candidates", "kernel.init_resolve"], reps),
       "version": orb.version()}
print(json.dumps(out))

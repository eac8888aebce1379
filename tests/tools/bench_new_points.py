#!/usr/bin/env python3
"""Latency of ft_search_and_triangulate on an MI355X (not part of the test suite), on the two shapes of bench_triangulation.py:
keyframes of 2 000 features, FeatureVectors from a k = 10, L = 5 tree at levelsup 4; 10 pinhole neighbours and 30 two-camera
KannalaBrandt8 neighbours.
usage: tests/tools/bench_new_points.py [--reps N] [--parent-lib PATH] [--out profiles/new_points_bench.json]

Per shape, wall times (median [10th, 90th percentile] over the repetitions, ms) of ft_search_and_triangulate, of
ft_search_for_triangulation on this build and - with --parent-lib, a libfasttrack_amd.so built from the parent commit and loaded
beside this one into the same process - of the parent's ft_search_for_triangulation, the three timed alternately, repetition by
repetition, all three through ctypes on argument arrays built once; then the library's own timers, the HIP-event times of the three kernels (a run of their own), the stand-alone
ft_triangulate_new_points on the downloaded rows, and the launch / copy counts.  No time is a pass criterion."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import _capi, orb  # noqa: E402
from tests import new_points_cases as nc  # noqa: E402
from tests import triangulation_cases as tc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--features", type=int, default=2000)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = orb.Context(0)  # loads this build first: it decides the process's hardware-queue setting
res = dict(library=orb.version(), device=ctx.device_name, features=args.features, vocabulary="k 10, L 5, levelsup 4", reps=args.reps,
           parent_library=None, shapes=[])

parent = None
if args.parent_lib:
    P = C.CDLL(args.parent_lib, mode=os.RTLD_LOCAL | os.RTLD_NOW | getattr(os, "RTLD_DEEPBIND", 0))
    vp, i = C.c_void_p, C.c_int
    P.ft_version.restype = C.c_char_p
    P.ft_context_create.argtypes = [i, i, C.POINTER(vp)]
    P.ft_context_destroy.argtypes = [vp]
    P.ft_search_for_triangulation.argtypes = [vp, C.POINTER(_capi.TriangKeyFrame), i, C.POINTER(_capi.TriangKeyFrame), C.POINTER(_capi.TriangPair),
                                              i, i, i, vp, vp, vp]
    assert not hasattr(P, "ft_search_and_triangulate"), "--parent-lib is not a parent build: it has the new entry point"
    ph = vp()
    assert P.ft_context_create(0, 0, C.byref(ph)) == 0
    parent = (P, ph)
    res["parent_library"] = P.ft_version().decode()


def pct(ts):
    return [round(float(np.median(ts)), 4), round(float(np.percentile(ts, 10)), 4), round(float(np.percentile(ts, 90)), 4)]


def stat_ms(name):
    total, calls = ctx.get_stat(name)
    return round(total / max(calls, 1), 4)


for form, nn in (("pinhole", 10), ("kb8x2", 30)):
    S = tc.scenario.__wrapped__(form, 5, n=args.features, neighbours=5, levelsup=4, vocab=(10, 5, 3))
    kf1 = tc.to_device(orb, S["kf1"])
    g1 = nc.to_device_geometry(orb, nc.geometry_from_pair(S["kf1"], S["pairs"][0], True))
    k5 = [tc.to_device(orb, k) for k in S["neighbours"]]
    g5 = [nc.to_device_geometry(orb, nc.geometry_from_pair(k, p, False)) for k, p in zip(S["neighbours"], S["pairs"])]
    p5 = [tc.to_device_pair(orb, p) for p in S["pairs"]]
    k2, g2, ps = [k5[j % 5] for j in range(nn)], [g5[j % 5] for j in range(nn)], [p5[j % 5] for j in range(nn)]
    kw = dict(inertial=False, far_points=True, th_far_points=40.0, ratio_factor=nc.RATIO_FACTOR)
    fused = lambda: orb.search_and_triangulate(ctx, kf1, g1, k2, g2, ps, **kw)
    search = lambda: orb.search_for_triangulation(ctx, kf1, k2, ps)
    # the timed calls go to the C entry points with argument arrays built once: the same path into this build and into the parent's
    n1 = kf1.c.n
    K2 = (_capi.TriangKeyFrame * nn)(*[k.c for k in k2])
    G2 = (_capi.NewPointGeometry * nn)(*[g.c for g in g2])
    PP = (_capi.TriangPair * nn)(*ps)
    cnt, mflat, bflat = np.zeros(nn, np.int32), np.full(nn * n1, -1, np.int32), np.full(nn * n1, 50, np.int32)
    st_, x3_, np_, first_ = np.zeros(nn * n1, np.int32), np.zeros(nn * n1 * 3, np.float32), np.zeros(nn, np.int32), np.zeros(n1, np.int32)
    L, ptr = _capi.lib(), _capi.ptr

    def raw_fused():
        assert L.ft_search_and_triangulate(ctx._h, C.byref(kf1.c), C.byref(g1.c), nn, K2, G2, PP, 0, 0, 1, 0, 1, 40.0, nc.RATIO_FACTOR, ptr(mflat),
                                           ptr(cnt), ptr(bflat), ptr(st_), ptr(x3_), ptr(np_), ptr(first_)) == 0

    def raw_search(lib=L, h=ctx._h):
        assert lib.ft_search_for_triangulation(h, C.byref(kf1.c), nn, K2, PP, 0, 0, 1, ptr(mflat), ptr(cnt), ptr(bflat)) == 0

    calls = [raw_fused, raw_search]
    if parent:
        calls.append(lambda: raw_search(parent[0], parent[1]))
    f, s = fused(), search()
    assert np.array_equal(f["matches12"], s["matches12"])
    raw_fused()
    assert np.array_equal(st_.reshape(nn, n1), f["status"]) and np.array_equal(mflat.reshape(nn, n1), s["matches12"])
    if parent:
        mflat[:] = -2
        calls[2]()
        assert np.array_equal(mflat.reshape(nn, n1), s["matches12"]), "the parent's matcher gives other rows"
    ctx.set_kernel_timing(False)
    ts = [[] for _ in calls]
    for _ in range(args.reps):
        for c, t in zip(calls, ts):
            t0 = time.perf_counter()
            c()
            t.append((time.perf_counter() - t0) * 1e3)
    ctx.reset_stats()
    for _ in range(args.reps):
        raw_fused(), raw_search()
    own_fused, own_search = stat_ms("search_and_triangulate.total"), stat_ms("search_for_triangulation.total")
    launches = (ctx.get_stat("search_and_triangulate.launches")[0] / args.reps, ctx.get_stat("search_for_triangulation.launches")[0] / args.reps)
    a = orb.triangulate_new_points(ctx, kf1, g1, k2, g2, s["matches12"], **kw)
    assert np.array_equal(a["status"], f["status"]) and np.array_equal(a["x3d"], f["x3d"])
    rows_in = np.ascontiguousarray(s["matches12"]).reshape(-1)

    def alone():
        assert L.ft_triangulate_new_points(ctx._h, C.byref(kf1.c), C.byref(g1.c), nn, K2, G2, ptr(rows_in), 0, 1, 40.0, nc.RATIO_FACTOR, ptr(st_),
                                           ptr(x3_), ptr(np_), ptr(first_)) == 0
    ta = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        alone()
        ta.append((time.perf_counter() - t0) * 1e3)
    ctx.set_kernel_timing(True)
    ctx.reset_stats()
    for _ in range(args.reps):
        raw_fused()
    km, kf, kp = stat_ms("kernel.triang_match"), stat_ms("kernel.triang_finish"), stat_ms("kernel.triang_points")
    ctx.set_kernel_timing(False)
    st = f["status"]
    shape = dict(form=form, neighbours=nn, features_kf1=len(S["kf1"]["keys"]), slots=int(st.size), matches=int(f["n"].sum()),
                 match_fraction=round(float(f["n"].sum()) / st.size, 4), points=int(f["n_points"].sum()),
                 triangulated=int((st == 1).sum()), past_the_branch=int(((st >= 1) | (st <= -3)).sum()),
                 status_counts={str(v): int(c) for v, c in zip(*np.unique(st, return_counts=True))},
                 fused_wall_ms=pct(ts[0]), search_wall_ms=pct(ts[1]), parent_search_wall_ms=pct(ts[2]) if parent else None,
                 fused_minus_parent_search_ms=round(float(np.median(ts[0]) - np.median(ts[2])), 4) if parent else None,
                 fused_minus_search_ms=round(float(np.median(ts[0]) - np.median(ts[1])), 4), fused_library_ms=own_fused,
                 search_library_ms=own_search, standalone_wall_ms=pct(ta), kernel_triang_match_ms=km, kernel_triang_finish_ms=kf,
                 kernel_triang_points_ms=kp, launches_fused=launches[0], launches_search=launches[1], copies_fused="1 up, 1 down",
                 copies_search_then_standalone="2 up, 2 down")
    res["shapes"].append(shape)
    print(json.dumps(shape), flush=True)
if parent:
    parent[0].ft_context_destroy(parent[1])
line = json.dumps(res)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
print(line)

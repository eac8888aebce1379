#!/usr/bin/env python3
"""Latency of ft_distinctive_descriptors on an MI355X (not part of the test suite): one call for the map points of a Local Mapping
step.
usage: tests/tools/bench_distinct.py [--points 1000] [--reps N] [--seed S] [--out profiles/distinct_bench.json]

The workload: `--points` map points whose list lengths are drawn (numpy default_rng(seed)) as: with probability 0.9 uniform in
2 .. 12, otherwise 12 + a geometric tail (p = 0.06) cut at 100.  Every list is a random base descriptor with up to 30 flipped bits per
row.  Timed, each as the median / 10th / 90th percentile over the repetitions of the host clock around the call (which ends in its
stream synchronise):
  batched          one call for all the points;
  single_calls     the same points as `--points` one-point calls of the same entry point;
  host_loop        the reference's loop (src/MapPoint.cc:368-397: the float matrix, a sorted copy of each row, the strict <) as plain
                   C++, written below, compiled with g++ -O2 and run on one host core over the same packed arrays;
  all_64           one call with every list at 64 descriptors (the wave class only);
and, from runs of their own, the library's own timer and the HIP-event times of the kernels of the batched call.  The batched and
the single calls are timed alternately.  Before anything is timed the batched result is compared with the restatement
(tests/distinct_ref.py) and the host loop with both."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from tests import distinct_cases as dc  # noqa: E402
from tests import distinct_ref as dr  # noqa: E402

HOST_LOOP = r"""
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>
static int descriptorDistance(const uint8_t *a, const uint8_t *b) {  // ORBmatcher::DescriptorDistance: 8 x 32 bits
    int dist = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t x, y;
        memcpy(&x, a + 4 * i, 4);
        memcpy(&y, b + 4 * i, 4);
        unsigned v = x ^ y;
        v = v - ((v >> 1) & 0x55555555);
        v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
        dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
    }
    return dist;
}
extern "C" void host_loop(int nPoints, const int *offsets, const uint8_t *desc, int *bestIdx, int *bestMedian, uint8_t *out) {
    std::vector<float> Distances;
    for (int p = 0; p < nPoints; p++) {
        const size_t N = (size_t)(offsets[p + 1] - offsets[p]);
        const uint8_t *v = desc + 32 * (size_t)offsets[p];
        bestIdx[p] = bestMedian[p] = -1;
        if (N == 0) continue;
        Distances.assign(N * N, 0.f);
        for (size_t i = 0; i < N; i++) {
            Distances[i * N + i] = 0;
            for (size_t j = i + 1; j < N; j++) {
                int distij = descriptorDistance(v + 32 * i, v + 32 * j);
                Distances[i * N + j] = distij;
                Distances[j * N + i] = distij;
            }
        }
        int BestMedian = INT_MAX, BestIdx = 0;
        for (size_t i = 0; i < N; i++) {
            std::vector<int> vDists(Distances.begin() + i * N, Distances.begin() + (i + 1) * N);
            std::sort(vDists.begin(), vDists.end());
            int median = vDists[0.5 * (N - 1)];
            if (median < BestMedian) {
                BestMedian = median;
                BestIdx = i;
            }
        }
        bestIdx[p] = BestIdx;
        bestMedian[p] = BestMedian;
        memcpy(out + 32 * (size_t)p, v + 32 * (size_t)BestIdx, 32);
    }
}
"""

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=1000)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = orb.Context(0)
rng = np.random.default_rng(args.seed)
P = args.points
lengths = np.where(rng.random(P) < 0.9, rng.integers(2, 13, P), np.minimum(12 + rng.geometric(0.06, P), 100)).astype(int)
lists = [dc.near(int(rng.integers(0, 1 << 30)), int(n), flips=30) for n in lengths]
offsets, desc = dc.pack(lists)
lists64 = [dc.near(int(rng.integers(0, 1 << 30)), 64, flips=30) for _ in range(P)]
offsets64, desc64 = dc.pack(lists64)

tmp = tempfile.mkdtemp()
with open(os.path.join(tmp, "host_loop.cpp"), "w") as f:
    f.write(HOST_LOOP)
subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(tmp, "host_loop.cpp"), "-o", os.path.join(tmp, "host_loop.so")])
host = C.CDLL(os.path.join(tmp, "host_loop.so"))
vp = C.c_void_p
host.host_loop.argtypes = [C.c_int, vp, vp, vp, vp, vp]
h_idx, h_med, h_out = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros((P, 32), np.uint8)


def host_loop(o=offsets, d=desc):
    host.host_loop(P, o.ctypes.data_as(vp), d.ctypes.data_as(vp), h_idx.ctypes.data_as(vp), h_med.ctypes.data_as(vp), h_out.ctypes.data_as(vp))


want = dr.distinctive_descriptors(offsets, desc)
got = ctx.distinctive_descriptors(offsets, desc)
assert all(np.array_equal(g, w) for g, w in zip(got, want)), "the batched call differs from the restatement"
host_loop()
assert np.array_equal(h_idx, want[0]) and np.array_equal(h_med, want[1]) and np.array_equal(h_out, want[2]), "the host loop differs"
want64 = dr.distinctive_descriptors(offsets64, desc64)
assert all(np.array_equal(g, w) for g, w in zip(ctx.distinctive_descriptors(offsets64, desc64), want64)), "all_64 differs from the restatement"

singles_in = [dc.pack([v]) for v in lists]
batched = lambda: ctx.distinctive_descriptors(offsets, desc)
singles = lambda: [ctx.distinctive_descriptors(o, d) for o, d in singles_in]
all64 = lambda: ctx.distinctive_descriptors(offsets64, desc64)


def clock(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def spread(ts):
    return dict(median=round(float(np.median(ts)), 4), p10=round(float(np.percentile(ts, 10)), 4), p90=round(float(np.percentile(ts, 90)), 4))


def stat_ms(name):
    total, calls = ctx.get_stat(name)
    return round(total / max(calls, 1), 4)


def library_and_kernels(fn, reps):
    ctx.set_kernel_timing(False)
    ctx.reset_stats()
    for _ in range(reps):
        fn()
    own = stat_ms("distinctive_descriptors.total")
    launches = ctx.get_stat("distinctive_descriptors.launches")
    ctx.set_kernel_timing(True)
    ctx.reset_stats()
    for _ in range(reps):
        fn()
    k = {n: stat_ms("kernel.distinct_" + n) for n in ("short", "wave", "block") if ctx.get_stat("kernel.distinct_" + n)[1]}
    ctx.set_kernel_timing(False)
    return own, launches[0] / max(launches[1], 1), k


for _ in range(3):
    batched(), all64(), host_loop()
singles()
tb, ts = [], []
single_reps = max(args.reps // 10, 5)
for r in range(args.reps):  # alternately: what else runs on the host hits both alike
    tb.append(clock(batched))
    if r < single_reps:
        ts.append(clock(singles))
th = [clock(host_loop) for _ in range(args.reps)]
t64 = [clock(all64) for _ in range(args.reps)]
th64 = [clock(lambda: host_loop(offsets64, desc64)) for _ in range(max(args.reps // 10, 5))]
own, launches, kernels = library_and_kernels(batched, args.reps)
own64, launches64, kernels64 = library_and_kernels(all64, args.reps)
classes = dict(le_8=int((lengths <= 8).sum()), le_16=int(((lengths > 8) & (lengths <= 16)).sum()),
               le_64=int(((lengths > 16) & (lengths <= 64)).sum()), longer=int((lengths > 64).sum()))
res = dict(library=orb.version(), device=ctx.device_name, points=P, seed=args.seed, reps=args.reps,
           lengths=dict(distribution="p 0.9: uniform 2 .. 12; else 12 + geometric(0.06), cut at 100", median=float(np.median(lengths)),
                        p90=float(np.percentile(lengths, 90)), max=int(lengths.max()), descriptors=int(offsets[-1]), classes=classes,
                        distance_pairs=int((lengths * (lengths - 1) // 2).sum())),
           batched=dict(wall_ms=spread(tb), library_ms=own, launches=launches, kernels_ms=kernels, bytes_up=int(32 * offsets[-1] + 16 * P),
                        bytes_down=int(40 * P)),
           single_calls=dict(wall_ms=spread(ts), calls=P, reps=single_reps),
           host_loop=dict(wall_ms=spread(th), what="src/MapPoint.cc:368-397 as plain C++, g++ -O2, one core, the same packed arrays"),
           all_64=dict(wall_ms=spread(t64), library_ms=own64, launches=launches64, kernels_ms=kernels64, descriptors=64 * P,
                       host_loop_wall_ms=spread(th64)))
line = json.dumps(res)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
print(line)

#!/usr/bin/env python3
"""Long randomized parity run of MapPoint::ComputeDistinctiveDescriptors on an MI355X (not part of the test suite):
ft_distinctive_descriptors against the sequential restatement (tests/distinct_ref.py).
usage: tests/tools/soak_distinct.py [--trials N] [--seed S] [--out profiles/distinct_soak.txt]

A trial is one call of 1 .. 400 points.  A point's list length is drawn from a mix of the length classes: mostly 1 .. 16, the edges
7 - 9, 15 - 17 and 63 - 65, lists up to 64, now and then one of 65 .. 400 and, rarely, one up to the cap; every tenth list is empty.
A list is either one base descriptor with up to f flipped bits per row (f drawn per list from 0 .. 40: medians tie often), random
descriptors, or a base and its complement mixed (distances of 256).  best_index, best_median and the 32 bytes must be equal, the rows of
points with an empty list must keep the sentinel, and every fifth trial is repeated with the optional outputs NULL.  Prints one line
per failure and a summary; exit code 1 on any mismatch."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb  # noqa: E402
from tests import distinct_cases as dc  # noqa: E402
from tests import distinct_ref as dr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=60)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--out", default=None)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
ctx = orb.Context(0)
SENTINEL = 0x5A


def draw_length():
    u = rng.random()
    if u < 0.10:
        return 0
    if u < 0.55:
        return int(rng.integers(1, 17))
    if u < 0.70:
        return int(rng.choice([7, 8, 9, 15, 16, 17, 63, 64, 65]))
    if u < 0.95:
        return int(rng.integers(17, 65))
    if u < 0.995:
        return int(rng.integers(65, 401))
    return int(rng.integers(401, dc.CAP + 1))


def draw_list(n):
    seed = int(rng.integers(0, 1 << 30))
    kind = rng.random()
    if n == 0:
        return dc.EMPTY
    if kind < 0.6:
        return dc.near(seed, n, flips=int(rng.integers(0, 41)))
    if kind < 0.9:
        return dc.spread(seed, n)
    v = dc.near(seed, n, flips=3)
    flip = rng.random(n) < 0.5
    v[flip] = np.bitwise_not(v[flip])
    return v


calls = points = mismatches = ties = at_256 = 0
by_class = [0, 0, 0, 0, 0]  # empty, <= 8, <= 16, <= 64, longer
longest = 0
t0 = time.time()
for trial in range(args.trials):
    lists = [draw_list(draw_length()) for _ in range(int(rng.integers(1, 401)))]
    offsets, desc = dc.pack(lists)
    sentinel = np.full((len(lists), 32), SENTINEL, np.uint8)
    want = dr.distinctive_descriptors(offsets, desc, sentinel)
    got = ctx.distinctive_descriptors(offsets, desc, sentinel.copy())
    calls += 1
    bad = [name for name, g, w in zip(("best_index", "best_median", "descriptors"), got, want) if not np.array_equal(g, w)]
    if trial % 5 == 0:
        only = ctx.distinctive_descriptors(offsets, desc, want_median=False, want_descriptors=False)
        bad += ["best_index with NULL outputs"] if not np.array_equal(only[0], want[0]) else []
    if bad:
        mismatches += 1
        print(f"MISMATCH trial {trial}: {bad}, lengths {[len(v) for v in lists]}")
    points += len(lists)
    for v in lists:
        n = len(v)
        by_class[0 if n == 0 else 1 if n <= 8 else 2 if n <= 16 else 3 if n <= 64 else 4] += 1
        longest = max(longest, n)
        if 0 < n <= 64:  # what the restatement saw: ties of the smallest median, rows with a distance of 256
            D = np.array(dr.distance_matrix(v))
            med = np.sort(D, axis=1)[:, (n - 1) // 2]
            ties += int((med == med.min()).sum() > 1)
            at_256 += int((D == 256).any())
line = (f"distinctive descriptors soak: seed {args.seed}, {calls} calls, {points} points, {mismatches} mismatches; lists: {by_class[0]} empty, "
        f"{by_class[1]} of 1 - 8, {by_class[2]} of 9 - 16, {by_class[3]} of 17 - 64, {by_class[4]} longer (longest {longest}); among the lists "
        f"of up to 64 the restatement saw {ties} with a tie of the smallest median and {at_256} with a distance of 256; {orb.version()} on "
        f"{ctx.device_name}, {time.time() - t0:.0f} s")
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
sys.exit(1 if mismatches else 0)

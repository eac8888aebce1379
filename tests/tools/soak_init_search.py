#!/usr/bin/env python3
"""Long randomized parity run of ORBmatcher::SearchForInitialization on an MI355X (not part of the test suite):
ft_search_for_initialization and ft_tracked_frame_search_for_initialization against the restatement (tests/init_search_ref.py).
usage: tests/tools/soak_init_search.py [--trials N] [--seed S]

A trial draws a frame size, a feature count, a scene and a displacement, extracts the two frames with the oracle, and either
keeps their descriptors or draws both from a small dictionary with a few flipped bits (ties, evictions and ratio failures
everywhere); window, ratio, orientation check and a perturbation of vbPrevMatched are random.  vnMatches12, vbPrevMatched (as
bits), nmatches and vMatchedDistance must be equal.  Prints one line per failure and a summary; exit code 1 on any mismatch."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fasttrack_amd import orb, synth  # noqa: E402
from oracle import binding as ob  # noqa: E402
from tests import init_search_ref as ref  # noqa: E402
from tests import scenarios as sc  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dictionary_descriptors(rng, n1, n2):
    words = int(rng.integers(3, 24))
    dic = rng.integers(0, 256, (words, 32), dtype=np.uint8)
    for wd in range(1, words):
        dic[wd] = dic[0]
        for b in rng.choice(256, int(rng.integers(5, 40)), replace=False):
            dic[wd, b // 8] ^= 1 << (b % 8)
    out = []
    for n in (n1, n2):
        d = dic[rng.integers(0, words, n)].copy()
        for i in range(n):
            for b in rng.choice(256, int(rng.integers(0, 4)), replace=False):
                d[i, b // 8] ^= 1 << (b % 8)
        out.append(d)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args(argv)
    rng = np.random.default_rng(a.seed)
    sf, _ = ob.scale_factors(1.2, 8)
    ctx = orb.Context(0)
    ini, cur = orb.TrackedFrame(ctx, 12000, 1), orb.TrackedFrame(ctx, 12000, 1)
    bad = calls = 0
    totals = dict(evictions=0, skipped=0, removed_by_histogram=0, evicted_in_kept_bin=0, matches=0)
    t0 = time.time()
    for trial in range(a.trials):
        w, h = [(752, 480), (640, 480), (512, 512), (320, 240), (1280, 720)][int(rng.integers(0, 5))]
        nf = int(rng.choice([500, 1500, 5000, 10000])) if w < 1280 else int(rng.choice([2500, 10000]))
        seed = int(rng.integers(0, 1 << 30))
        kind = int(rng.integers(0, 3))
        base = synth.make_image(w, h, seed) if kind < 2 else synth.make_mosaic_pair(w, h, seed, block=int(rng.integers(8, 20)))[0]
        dx, dy = int(rng.integers(-40, 41)), int(rng.integers(-40, 41))
        moved = np.roll(base, (dy, dx), axis=(0, 1)).astype(np.int32) + rng.integers(-3, 4, base.shape)
        moved = np.ascontiguousarray(np.clip(moved, 0, 255).astype(np.uint8))
        k1, d1, _ = ob.Extractor(nf).extract(base, (0, 1000))
        k2, d2, _ = ob.Extractor(nf).extract(moved, (0, 1000))
        if rng.random() < 0.2:  # N1 != N2 by a lot; sometimes no level-0 keypoint on one side
            keep = k2["octave"] > 0 if rng.random() < 0.3 else rng.random(len(k2)) < 0.6
            k2, d2 = k2[keep], d2[keep]
        if kind == 1:
            d1, d2 = dictionary_descriptors(rng, len(k1), len(k2))
        bounds = sc.frame_bounds(w, h)
        o2, g2 = ob.FrameView(k2, d2, sf, bounds), orb.FrameView(k2, d2, sf, bounds)
        g1 = orb.FrameView(k1, d1, sf, bounds)
        ini.upload(g1)
        cur.upload(g2)
        prev = np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32)
        for step in range(int(rng.integers(1, 4))):  # chained: the call's vbPrevMatched feeds the next one
            window = int(rng.choice([5, 15, 30, 100, 100, 250, 3000]))
            ratio = float(rng.choice([0.6, 0.9, 0.9, 1.0, 1.5]))
            ori = bool(rng.random() < 0.7)
            if rng.random() < 0.3:
                sel = rng.random(len(prev)) < 0.2
                prev = prev.copy()
                prev[sel] += rng.choice(np.array([-300.0, -20.5, 7.25, 64.0, 2000.0], np.float32), (int(sel.sum()), 2))
            o = ref.search_for_initialization(k1, d1, o2, prev, window, ratio, ori)
            g = orb.KernelController.search_for_initialization(ctx, g1, g2, prev, window, ratio, ori)
            t = cur.search_for_initialization(ini, prev, window, ratio, ori)
            calls += 2
            for tag, r in (("non-resident", g), ("resident", t)):
                why = None
                if r["n"] != o["n"]:
                    why = "n %d vs %d" % (r["n"], o["n"])
                elif not np.array_equal(r["matches12"], o["matches12"]):
                    why = "matches12"
                elif not np.array_equal(bits(r["prev_matched"]), bits(o["prev_matched"])):
                    why = "prev_matched"
                elif tag == "non-resident" and not np.array_equal(r["matched_distance"], o["matched_distance"]):
                    why = "matched_distance"
                if why:
                    bad += 1
                    print(f"MISMATCH trial {trial} step {step} {tag}: {why}  ({w}x{h} nf {nf} seed {seed} kind {kind} shift {dx},{dy} "
                          f"window {window} ratio {ratio} ori {ori} N1 {len(k1)} N2 {len(k2)})", flush=True)
            for key in ("evictions", "skipped", "removed_by_histogram", "evicted_in_kept_bin"):
                totals[key] += o["stats"][key]
            totals["matches"] += o["n"]
            prev = o["prev_matched"]
    print(f"soak_init_search: trials {a.trials} calls {calls} mismatches {bad} seed {a.seed} {totals} "
          f"{time.time() - t0:.0f} s  {orb.version()}")
    ini.close()
    cur.close()
    ctx.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

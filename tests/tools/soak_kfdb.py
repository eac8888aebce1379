"""Randomized add / erase / clear / query sequences on the device-resident KeyFrameDatabase against the sequential restatement
(tests/kfdb_ref.py): every output of every query, the doubles before the rounding included, and the state of both kinds in every
live keyframe after it, bit for bit; the two selection calls behind every query with random neighbours and maps.
usage: python tests/tools/soak_kfdb.py [--trials 60] [--seed 1] [--out profiles/kfdb_soak.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from fasttrack_amd import orb  # noqa: E402
from tests import kfdb_cases as kc  # noqa: E402
from tests import kfdb_ref as kr  # noqa: E402


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=60)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfdb_soak.txt"))
    a = ap.parse_args()
    ctx = orb.Context(0)
    n = dict(queries=0, listed=0, scored=0, adds=0, erased=0, clears=0, candidates=0, mismatches=0)
    for t in range(a.trials):
        ops = kc.random_case(a.seed * 1000 + t, n_ops=14)
        db, ref = orb.KeyFrameDatabase(ctx), kr.KeyFrameDatabase()
        for k, op in enumerate(ops):
            got, want = kc.replay(db, op), kc.replay(ref, op)
            if op[0] == "add":
                n["adds"] += len(want)
                n["mismatches"] += got != want
            elif op[0] == "erase":
                n["erased"] += len(op[1])
            elif op[0] == "clear":
                n["clears"] += 1
            else:
                kind, qid = op[1], op[2]
                n["queries"] += 1
                n["listed"] += want["n_sharing"]
                n["scored"] += len(want["handles"])
                bad = any(got[key] != want[key] for key in ("n_sharing", "max_common_words", "min_common_words"))
                bad |= any(not np.array_equal(bits(got[key]), bits(want[key])) for key in ("handles", "words", "scores", "raw_scores"))
                live = sorted(ref.keyframes)
                for kd in (0, 1):
                    bad |= any(not np.array_equal(bits(g), bits(w)) for g, w in zip(db.state(kd, live), ref.state(kd, live)))
                rng = np.random.default_rng([a.seed, t, k])
                table = {h: [int(x) for x in rng.choice(live, size=min(len(live), int(rng.integers(0, 11))), replace=False)] for h in live}
                maps = (lambda h: h % 3)
                if kind == kc.PLACE:
                    w2 = ref.select_n_best(qid, want, table.__getitem__, maps, 0, 3, (2,))
                    g2 = db.select_n_best(qid, got, table.__getitem__, maps, 0, 3, (2,))
                    bad |= [x.tolist() for x in g2] != [list(x) for x in w2]
                    n["candidates"] += len(w2[0]) + len(w2[1])
                else:
                    w2 = ref.select_reloc(qid, want, table.__getitem__, maps, 0)
                    bad |= db.select_reloc(qid, got, table.__getitem__, maps, 0).tolist() != list(w2)
                    n["candidates"] += len(w2)
                if bad:
                    n["mismatches"] += 1
                    print("MISMATCH trial %d op %d" % (t, k))
        db.close()
    compactions = ctx.get_stat("kfdb.compactions")[1]
    ctx.close()
    line = ("soak_kfdb: library %s, seed %d, %d trials: %d queries (%d listed, %d scored keyframes, %d candidates selected), %d keyframes added, "
            "%d erased, %d clears, %d compactions: %d mismatches" % (orb.version(), a.seed, a.trials, n["queries"], n["listed"], n["scored"],
                                                                       n["candidates"], n["adds"], n["erased"], n["clears"], compactions, n["mismatches"]))
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(line + "\n")
    return 1 if n["mismatches"] else 0


if __name__ == "__main__":
    sys.exit(main())

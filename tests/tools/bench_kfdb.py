"""Times the scoring call of the device-resident KeyFrameDatabase (ft_kfdb_score) against a plain sequential C++ restatement
of the same part of DetectNBestCandidates (src/KeyFrameDatabase.cc:615-666: std::list per word, std::map BowVectors, as the
reference holds them), compiled -O3 inside this tool and run on one host core.

Databases of 1 000 and 5 000 keyframes of about 1 200 words over a 10^6-word id space; queries of 1 200 words that revisit a stored
place (they keep about 60 % of a stored keyframe's words).  Both sides answer the same queries with fresh ids on the same database;
their n_sharing / n_scored and the float scores are compared before anything is timed.  Wall = host clock around the call (which
ends in a device synchronise); median [10th, 90th percentile] after a warm-up; kernel times are HIP events in a pass of their own.

usage: python tests/tools/bench_kfdb.py [--reps 200] [--out profiles/kfdb_bench.json]"""
import argparse
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

W = 1_000_000

CPP = r"""
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <vector>
typedef std::map<unsigned, double> BowVector;
struct KeyFrame { BowVector mBowVec; long mnPlaceRecognitionQuery = 0; int mnPlaceRecognitionWords = 0; float mPlaceRecognitionScore = 0; };
static double score(const BowVector &v1, const BowVector &v2) {
    BowVector::const_iterator a = v1.begin(), b = v2.begin();
    double s = 0;
    while (a != v1.end() && b != v2.end()) {
        if (a->first == b->first) { s += fabs(a->second - b->second) - fabs(a->second) - fabs(b->second); ++a; ++b; }
        else if (a->first < b->first) a = v1.lower_bound(b->first);
        else b = v2.lower_bound(a->first);
    }
    return -s / 2.0;
}
static BowVector readVec(FILE *f) {
    int n = 0;
    if (fread(&n, 4, 1, f) != 1) n = 0;
    std::vector<unsigned> ids(n);
    std::vector<double> vals(n);
    if (n && (fread(ids.data(), 4, n, f) != (size_t)n || fread(vals.data(), 8, n, f) != (size_t)n)) n = 0;
    BowVector v;
    for (int i = 0; i < n; i++) v.insert(v.end(), std::make_pair(ids[i], vals[i]));
    return v;
}
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb");
    const int reps = atoi(argv[2]);
    int nKf = 0, nQ = 0, nWords = 0;
    if (fread(&nWords, 4, 1, f) != 1 || fread(&nKf, 4, 1, f) != 1 || fread(&nQ, 4, 1, f) != 1) return 1;
    std::vector<KeyFrame *> kfs;
    std::vector<std::list<KeyFrame *>> mvInvertedFile(nWords);
    for (int k = 0; k < nKf; k++) {
        KeyFrame *kf = new KeyFrame;
        kf->mBowVec = readVec(f);
        for (auto &e : kf->mBowVec) mvInvertedFile[e.first].push_back(kf);
        kfs.push_back(kf);
    }
    std::vector<BowVector> queries;
    for (int q = 0; q < nQ; q++) queries.push_back(readVec(f));
    std::vector<double> ms;
    long id = 0;
    for (int r = -3; r < reps; r++) {
        const BowVector &Q = queries[(r + 3) % nQ];
        id++;
        const auto t0 = std::chrono::steady_clock::now();
        std::list<KeyFrame *> lKFsSharingWords;
        for (auto vit = Q.begin(); vit != Q.end(); vit++) {
            std::list<KeyFrame *> &lKFs = mvInvertedFile[vit->first];
            for (auto lit = lKFs.begin(); lit != lKFs.end(); lit++) {
                KeyFrame *pKFi = *lit;
                if (pKFi->mnPlaceRecognitionQuery != id) {
                    pKFi->mnPlaceRecognitionWords = 0;
                    pKFi->mnPlaceRecognitionQuery = id;
                    lKFsSharingWords.push_back(pKFi);
                }
                pKFi->mnPlaceRecognitionWords++;
            }
        }
        int maxCommonWords = 0, nscores = 0;
        for (KeyFrame *k : lKFsSharingWords) maxCommonWords = std::max(maxCommonWords, k->mnPlaceRecognitionWords);
        const int minCommonWords = maxCommonWords * 0.8f;
        std::list<std::pair<float, KeyFrame *>> lScoreAndMatch;
        for (KeyFrame *k : lKFsSharingWords)
            if (k->mnPlaceRecognitionWords > minCommonWords) {
                nscores++;
                const float si = score(Q, k->mBowVec);
                k->mPlaceRecognitionScore = si;
                lScoreAndMatch.push_back(std::make_pair(si, k));
            }
        const auto t1 = std::chrono::steady_clock::now();
        if (r >= 0) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        if (r >= -3 && r < nQ - 3) {  // the first pass over the queries: the answers, for the comparison with the device
            double sum = 0;
            for (auto &e : lScoreAndMatch) sum += e.first;
            printf("answer %d %d %d %d %.9g\n", (int)lKFsSharingWords.size(), maxCommonWords, minCommonWords, nscores, sum);
        }
    }
    std::sort(ms.begin(), ms.end());
    printf("times %.6f %.6f %.6f\n", ms[ms.size() / 2], ms[ms.size() / 10], ms[ms.size() * 9 / 10]);
    return 0;
}
"""


def make_database(n_kf, seed, n_queries=8):
    rng = np.random.default_rng(seed)
    idf = rng.uniform(0.5, 12.0, 4096)

    def vec(ids):
        v = rng.integers(1, 4, len(ids)) * idf[ids % 4096]
        return ids.astype(np.uint32), v / v.sum()

    kfs = [vec(np.unique(rng.integers(0, W, int(rng.integers(1100, 1300))))) for _ in range(n_kf)]
    queries = []
    for _ in range(n_queries):   # a revisit: about 60 % of a stored keyframe's words, the rest new - 1 200 words
        base = kfs[int(rng.integers(0, n_kf))][0]
        keep = base[rng.random(len(base)) < 0.6]
        ids = np.unique(np.concatenate([keep, rng.integers(0, W, 1200 - len(keep)).astype(np.uint32)]))
        queries.append(vec(ids))
    return kfs, queries


def percentiles(ms):
    ms = np.sort(np.array(ms))
    return [round(float(ms[len(ms) // 2]), 5), round(float(ms[len(ms) // 10]), 5), round(float(ms[len(ms) * 9 // 10]), 5)]


def run_host(tmp, exe, kfs, queries, reps):
    path = os.path.join(tmp, "db.bin")
    with open(path, "wb") as f:
        f.write(np.array([W, len(kfs), len(queries)], np.int32).tobytes())
        for ids, vals in kfs + queries:
            f.write(np.array([len(ids)], np.int32).tobytes() + ids.tobytes() + vals.tobytes())
    out = subprocess.check_output([exe, path, str(reps)]).decode().splitlines()
    answers = [[float(x) for x in l.split()[1:]] for l in out if l.startswith("answer")]
    times = [float(x) for x in [l for l in out if l.startswith("times")][0].split()[1:]]
    return answers, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfdb_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[1000, 5000])
    a = ap.parse_args()
    ctx = orb.Context(0)
    result = dict(tool="tests/tools/bench_kfdb.py", library=orb.version(), device=ctx.device_name, reps=a.reps, sizes=[])
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "kfdb_host.cpp"), os.path.join(tmp, "kfdb_host")
        open(src, "w").write(CPP)
        subprocess.check_call(["g++", "-O3", "-std=c++17", src, "-o", exe])
        for n_kf in a.sizes:
            kfs, queries = make_database(n_kf, 7 + n_kf)
            db = orb.KeyFrameDatabase(ctx)
            t0 = time.perf_counter()
            for k in range(0, n_kf, 250):
                db.add(kfs[k:k + 250])
            add_ms = (time.perf_counter() - t0) * 1e3
            host_answers, host_times = run_host(tmp, exe, kfs, queries, a.reps)
            qid = 0
            for q, want in zip(queries, host_answers):   # the same answers first (the host program numbers its queries 1, 2, ...)
                qid += 1
                r = db.score(orb.KeyFrameDatabase.PLACE, qid, *q)
                got = [r["n_sharing"], r["max_common_words"], r["min_common_words"], len(r["handles"])]
                assert got == [int(x) for x in want[:4]], (got, want)
                assert abs(float(np.sum(r["scores"].astype(np.float64))) - want[4]) < 1e-6 * max(1.0, want[4]), (r["scores"].sum(), want)
            for _ in range(20):                           # warm-up
                qid += 1
                db.score(orb.KeyFrameDatabase.PLACE, qid, *queries[qid % len(queries)])
            wall = []
            for _ in range(a.reps):
                qid += 1
                q = queries[qid % len(queries)]
                t0 = time.perf_counter()
                db.score(orb.KeyFrameDatabase.PLACE, qid, *q)
                wall.append((time.perf_counter() - t0) * 1e3)
            ctx.set_kernel_timing(True)
            ctx.reset_stats()
            for _ in range(50):
                qid += 1
                db.score(orb.KeyFrameDatabase.PLACE, qid, *queries[qid % len(queries)])
            kern = {k: round(ctx.get_stat("kernel.kfdb_" + k)[0] / 50, 5) for k in ("count", "score")}
            launches = ctx.get_stat("kfdb_score.launches")
            inside = ctx.get_stat("kfdb_score.total")
            ctx.set_kernel_timing(False)
            n_live, n_words = db.size()
            entry = dict(keyframes=n_live, stored_words=n_words, query_words=int(np.mean([len(q[0]) for q in queries])),
                         n_sharing=[int(x[0]) for x in host_answers], n_scored=[int(x[3]) for x in host_answers],
                         device_wall_ms=percentiles(wall), device_kernel_ms_with_events=kern,
                         device_inside_library_ms_with_events=round(inside[0] / inside[1], 5),
                         launches_per_call=launches[0] / launches[1], host_cpp_ms=[round(x, 5) for x in host_times],
                         add_ms_total=round(add_ms, 2), device_wins=bool(percentiles(wall)[0] < host_times[0]))
            result["sizes"].append(entry)
            print(json.dumps(entry))
            db.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(result, open(a.out, "w"))
    print("wrote", a.out)


if __name__ == "__main__":
    main()

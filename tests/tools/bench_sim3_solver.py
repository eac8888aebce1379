#!/usr/bin/env python3
"""Latency of ft_sim3_solver on an MI355X (not part of the test suite): calls of 1, 6 and 32 problems of 30, 100 and 300 pairs at
300 iterations (pinhole keyframes, the problems of tests/sim3_solver_cases.py), for a set that CONVERGES (half of the pairs planted
inliers, min_inliers a fifth of the pairs) and one that NEVER does (a fifth of the pairs inliers, min_inliers equal to them).
usage: tests/tools/bench_sim3_solver.py [--reps N] [--out profiles/sim3_solver_bench.json]

Per shape: wall time of the call through ctypes on argument arrays built once (median [10th, 90th percentile] over the
repetitions, ms), the library's own timer, the HIP-event times of the three kernels (a run of its own) - and the same problems
through the sequential loop of Sim3Solver::iterate on one host core: sim3_host.cpp below, the restatement's arithmetic ported to
plain C++ (float steps in the reference's order, the same Jacobi, libm's sinf / cosf / atan2f), compiled with g++ -O2
-ffp-contract=off and called through ctypes on gathered pairs; it stops at convergence as the reference does, where the device
evaluates every effective iteration.  Its counts must equal the device's.  No time is a pass criterion."""
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
from fasttrack_amd import _capi, orb  # noqa: E402
from tests import sim3_solver_cases as sc  # noqa: E402
from tests import sim3_solver_ref as ref  # noqa: E402

HOST_SRC = r"""
#include <cmath>
#include <cstring>
static inline float sum3(float a, float b, float c) { return a + (b + c); }
static inline float dot3(const float *a, const float *b) { return sum3(a[0] * b[0], a[1] * b[1], a[2] * b[2]); }
static void eig(const double N[16], float q[4]) {
    double A[16], V[16];
    for (int i = 0; i < 16; i++) A[i] = N[i], V[i] = i % 5 == 0;
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 3; p++)
            for (int r = p + 1; r < 4; r++) {
                const double apq = A[4 * p + r], app = A[5 * p], aqq = A[5 * r];
                if (apq == 0.0 || !(std::fabs(apq) > 1e-18 * (std::fabs(app) + std::fabs(aqq)))) continue;
                rotated = true;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                A[5 * p] = app - t * apq, A[5 * r] = aqq + t * apq, A[4 * p + r] = A[4 * r + p] = 0.0;
                for (int k = 0; k < 4; k++) {
                    if (k != p && k != r) {
                        const double akp = A[4 * k + p], akq = A[4 * k + r];
                        A[4 * k + p] = A[4 * p + k] = c * akp - s * akq;
                        A[4 * k + r] = A[4 * r + k] = s * akp + c * akq;
                    }
                    const double vkp = V[4 * k + p], vkq = V[4 * k + r];
                    V[4 * k + p] = c * vkp - s * vkq, V[4 * k + r] = s * vkp + c * vkq;
                }
            }
        if (!rotated) break;
    }
    int best = 0;
    for (int j = 1; j < 4; j++)
        if (A[5 * j] > A[5 * best]) best = j;
    const bool flip = V[best] < 0;
    for (int i = 0; i < 4; i++) q[i] = (float)(flip ? -V[4 * i + best] : V[4 * i + best]);
}
static void centroid(const float P[3][3], float Pr[3][3], float C[3]) {
    for (int k = 0; k < 3; k++) C[k] = sum3(P[0][k], P[1][k], P[2][k]) / 3.f;
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) Pr[i][k] = P[i][k] - C[k];
}
static void hypothesis(const float P1[3][3], const float P2[3][3], int fixScale, float T12[12], float T21[12]) {
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3], M[3][3];
    centroid(P1, Pr1, O1), centroid(P2, Pr2, O2);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[i][j] = sum3(Pr2[0][i] * Pr1[0][j], Pr2[1][i] * Pr1[1][j], Pr2[2][i] * Pr1[2][j]);
    const float N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0],
                N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2], N33 = -M[0][0] + M[1][1] - M[2][2],
                N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
    const double Nd[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    float q[4];
    eig(Nd, q);
    float vec[3] = {q[1], q[2], q[3]};
    const float nv = sqrtf(dot3(vec, vec)), ang = atan2f(nv, q[0]);
    if (nv != 0)
        for (int i = 0; i < 3; i++) vec[i] = 2.f * ang * vec[i] / nv;
    const float th2 = dot3(vec, vec);
    float imag, real;
    if (th2 < 1e-5f * 1e-5f) {
        imag = 0.5f - (float)(1.0 / 48.0) * th2 + (float)(1.0 / 3840.0) * (th2 * th2);
        real = 1.f - (float)(1.0 / 8.0) * th2 + (float)(1.0 / 384.0) * (th2 * th2);
    } else {
        const float th = sqrtf(th2), half = 0.5f * th;
        imag = sinf(half) / th, real = cosf(half);
    }
    const float w = real, x = imag * vec[0], y = imag * vec[1], z = imag * vec[2];
    const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const float R[9] = {1.f - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.f - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.f - (txx + tyy)};
    float s = 1.f;
    if (!fixScale) {
        float nom = 0, den = 0;
        for (int i = 0; i < 3; i++)
            for (int k = 0; k < 3; k++) {
                const float p3 = dot3(R + 3 * k, Pr2[i]), a = Pr1[i][k] * p3, b = p3 * p3;
                nom = (i || k) ? nom + a : a, den = (i || k) ? den + b : b;
            }
        s = (float)((double)nom / (double)den);
    }
    float sR[9], t[3];
    for (int i = 0; i < 9; i++) sR[i] = s * R[i];
    for (int i = 0; i < 3; i++) t[i] = O1[i] - dot3(sR + 3 * i, O2);
    const float inv = (float)(1.0 / (double)s);
    for (int i = 0; i < 3; i++) {
        float row[3];
        for (int j = 0; j < 3; j++) T12[4 * i + j] = sR[3 * i + j], T21[4 * i + j] = inv * R[3 * j + i], row[j] = -T21[4 * i + j];
        T12[4 * i + 3] = t[i], T21[4 * i + 3] = dot3(row, t);
    }
}
// pairs: 12 floats each (X1, max1, X2, max2, P1, P2); pinhole cameras; -> iterations run, *converged, *nBest; counts[it]
extern "C" int sim3_host(int N, const float *pairs, const float *cam1, const float *cam2, int fixScale, int minInliers, int eff, const int *draws,
                         int *converged, int *nBest, int *counts) {
    int best = 0, its = 0;
    *converged = 0;
    while (its < eff) {
        const int *d = draws + 3 * its++;
        const int r0 = (int)((double)d[0] / 2147483648.0 * N), r1 = (int)((double)d[1] / 2147483648.0 * (N - 1)), r2 = (int)((double)d[2] / 2147483648.0 * (N - 2));
        const int back1 = (N - 2 == r0) ? N - 1 : N - 2, idx[3] = {r0, r1 == r0 ? N - 1 : r1, r2 == r1 ? back1 : r2 == r0 ? N - 1 : r2};
        float P1[3][3], P2[3][3], T12[12], T21[12];
        for (int i = 0; i < 3; i++) memcpy(P1[i], pairs + 12 * idx[i], 12), memcpy(P2[i], pairs + 12 * idx[i] + 4, 12);
        hypothesis(P1, P2, fixScale, T12, T21);
        int n = 0;
        for (int i = 0; i < N; i++) {
            const float *p = pairs + 12 * i;
            float a[3], b[3];
            for (int k = 0; k < 3; k++) a[k] = dot3(T12 + 4 * k, p + 4) + T12[4 * k + 3], b[k] = dot3(T21 + 4 * k, p) + T21[4 * k + 3];
            const float d1x = p[8] - (cam1[0] * a[0] / a[2] + cam1[2]), d1y = p[9] - (cam1[1] * a[1] / a[2] + cam1[3]);
            const float d2x = (cam2[0] * b[0] / b[2] + cam2[2]) - p[10], d2y = (cam2[1] * b[1] / b[2] + cam2[3]) - p[11];
            n += (d1x * d1x + d1y * d1y < p[3]) && (d2x * d2x + d2y * d2y < p[7]);
        }
        counts[its - 1] = n;
        if (n >= best) {
            best = n;
            if (n > minInliers) {
                *converged = 1;
                break;
            }
        }
    }
    *nBest = best;
    return its;
}
"""

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=None)
args = ap.parse_args()
tmp = tempfile.mkdtemp()
with open(os.path.join(tmp, "sim3_host.cpp"), "w") as fh:
    fh.write(HOST_SRC)
subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(tmp, "sim3_host.cpp"), "-o", os.path.join(tmp, "libsim3_host.so")])
HOST = C.CDLL(os.path.join(tmp, "libsim3_host.so"))
ctx = orb.Context(0)
res = dict(library=orb.version(), device=ctx.device_name, reps=args.reps, iterations=300, shapes=[])


def pct(ts):
    return [round(float(np.median(ts)), 4), round(float(np.percentile(ts, 10)), 4), round(float(np.percentile(ts, 90)), 4)]


def stat_ms(name):
    total, calls = ctx.get_stat(name)
    return round(total / max(calls, 1), 4)


def host_args(P):
    """the gathered pairs of a problem as the device records, and the effective iteration count"""
    G = ref.gather(P)
    N = len(G["idx"])
    rec = np.zeros((N, 12), np.float32)
    rec[:, 0:3], rec[:, 3], rec[:, 4:7], rec[:, 7] = G["X1"], G["max1"], G["X2"], G["max2"]
    rec[:, 8:10], rec[:, 10:12] = np.array(G["P1"], np.float32), np.array(G["P2"], np.float32)
    return rec, ref.effective_iterations(P["probability"], P["min_inliers"], N, P["max_iterations"])


for kind in ("converging", "never"):
    for n_pairs in (30, 100, 300):
        n_in, n_min = (n_pairs // 2, n_pairs // 5) if kind == "converging" else (n_pairs // 5, n_pairs // 5)
        pool = [sc.problem(500 + s, n_pairs, n_in, min_inliers=n_min, max_iterations=300, scale=1.2) for s in range(8)]
        dev = [sc.to_device(orb, P) for P in pool]
        host = [host_args(P) for P in pool]
        for n_problems in (1, 6, 32):
            probs = [dev[p % 8] for p in range(n_problems)]
            Pa = (_capi.Sim3Problem * n_problems)(*[p.c for p in probs])
            R = (_capi.Sim3Result * n_problems)()
            inl = [np.zeros(n_pairs, np.uint8) for _ in probs]
            hyp = [np.zeros(300, np.int32) for _ in probs]
            I = (C.c_void_p * n_problems)(*[_capi.ptr(a) for a in inl])
            Hy = (C.c_void_p * n_problems)(*[_capi.ptr(a) for a in hyp])
            L = _capi.lib()

            def call():
                assert L.ft_sim3_solver(ctx._h, n_problems, Pa, R, I, None, Hy) == 0

            call()
            ctx.set_kernel_timing(False)
            ctx.reset_stats()
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call()
                ts.append((time.perf_counter() - t0) * 1e3)
            own = stat_ms("sim3_solver.total")
            ctx.set_kernel_timing(True)
            ctx.reset_stats()
            for _ in range(args.reps):
                call()
            kernels = {k: stat_ms("kernel.sim3_" + k) for k in ("hypotheses", "count", "select")}
            ctx.set_kernel_timing(False)
            # the sequential loop on one host core, on the same problems
            conv, nb, cnt = C.c_int(), C.c_int(), np.zeros(300, np.int32)
            hs, its_host, same = [], 0, True
            for rep in range(args.reps):
                t0 = time.perf_counter()
                for p in range(n_problems):
                    rec, eff = host[p % 8]
                    P = pool[p % 8]
                    its = HOST.sim3_host(n_pairs, _capi.ptr(rec), _capi.ptr(P["cam1"]), _capi.ptr(P["cam2"]), int(P["fix_scale"]), P["min_inliers"], eff,
                                         _capi.ptr(P["rand_draws"]), C.byref(conv), C.byref(nb), _capi.ptr(cnt))
                    if rep == 0:
                        its_host += its
                        same = same and its == R[p].iterations and bool(conv.value) == bool(R[p].converged) and nb.value == R[p].n_best_inliers \
                            and np.array_equal(cnt[:its], hyp[p][:its])
                hs.append((time.perf_counter() - t0) * 1e3)
            shape = dict(kind=kind, problems=n_problems, pairs=n_pairs, wall_ms=pct(ts), library_ms=own, kernel_ms=kernels, host_sequential_ms=pct(hs),
                         host_iterations=its_host, device_iterations=int(sum(R[p].effective_iterations for p in range(n_problems))),
                         converged=int(sum(R[p].converged for p in range(n_problems))), host_equals_device=bool(same),
                         launches=ctx.get_stat("sim3_solver.launches")[0] / args.reps)
            res["shapes"].append(shape)
            print(json.dumps(shape), flush=True)
line = json.dumps(res)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
print(line)

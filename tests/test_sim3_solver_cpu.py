"""The restatement of Sim3Solver (tests/sim3_solver_ref.py), which checks ft_sim3_solver on the device, pinned against things that
are independent of it: Horn's solution through numpy's float64 eigh, the planted transforms and inlier sets of the committed
cases, hand-computed iteration counts, a literal transcription of the reference's sampling loop and of iterate itself."""
import math

import numpy as np
import pytest

from tests import sim3_solver_cases as sc
from tests import sim3_solver_ref as ref

RUN = [k for k in sc.CASES if k not in sc.JOBLESS]
# (a) A sample is WELL CONDITIONED when the two largest eigenvalues of its N are separated by at least this fraction of the largest
# (a collinear or coincident sample has a repeated largest eigenvalue: its rotation about the line is free) and its scale is finite.
GAP = 0.05
# The largest deviations of a float32 hypothesis from float64 Horn over every well-conditioned hypothesis of the committed cases
# (505 of 545 hypotheses), as test_hypotheses_agree_with_horn_in_float64 prints them: R 1.3e-6 (absolute, per entry), s 4.7e-7
# (relative), t 5.7e-7 (relative to |t| + s |O2|, the size of the terms it is a difference of).  The bounds asserted are 4 x those.
HORN_MEASURED = dict(R=1.3e-6, s=4.7e-7, t=5.7e-7)
HORN_BOUND = {k: 4 * v for k, v in HORN_MEASURED.items()}


def horn64(P1, P2, fix_scale):
    """Horn 1987 in float64 with numpy.linalg.eigh -> R, s, t, the eigenvalues ascending"""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    O1, O2 = P1.mean(0), P2.mean(0)
    A, B = P1 - O1, P2 - O2
    M = B.T @ A
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, v = np.linalg.eigh(N)
    q = v[:, 3]
    a, b, c, d = q
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    P3 = B @ R.T
    with np.errstate(all="ignore"):
        s = 1.0 if fix_scale else (A * P3).sum() / (P3 * P3).sum()
    return R, s, O1 - s * R @ O2, w, O2


def test_hypotheses_agree_with_horn_in_float64():
    """(a) R, s, t of every well-conditioned hypothesis of every case against float64 Horn; HORN_MEASURED holds what this prints"""
    worst = dict(R=0.0, s=0.0, t=0.0)
    n_all = n_good = 0
    for key in RUN:
        P, want = sc.CASES[key], sc.reference(key)
        G = want["G"]
        for it, H in enumerate(want["hyps"]):
            i = ref.sample(P["rand_draws"][3 * it:3 * it + 3], len(G["idx"]))
            R, s, t, w, O2 = horn64([G["X1"][k] for k in i], [G["X2"][k] for k in i], P["fix_scale"])
            n_all += 1
            if not (w[3] > 0 and w[3] - w[2] >= GAP * w[3] and np.isfinite(H["s"])):
                continue
            n_good += 1
            worst["R"] = max(worst["R"], float(np.abs(H["R"].reshape(3, 3).astype(np.float64) - R).max()))
            worst["s"] = max(worst["s"], abs(float(H["s"]) - s) / s)
            tt = H["T12"].reshape(3, 4)[:, 3].astype(np.float64)
            worst["t"] = max(worst["t"], float(np.abs(tt - t).max() / (np.linalg.norm(t) + s * np.linalg.norm(O2))))
    print("horn:", n_good, "of", n_all, "hypotheses well conditioned; worst deviations", worst)
    assert n_good > 0.9 * n_all
    for k in worst:
        assert worst[k] <= HORN_BOUND[k], (k, worst[k])


def test_the_jacobi_eigenvector_is_eigh_s():
    """the eigenvector itself, on random symmetric matrices and on the committed hypotheses' N: float32 of eigh's, up to the sign"""
    rng = np.random.default_rng(5)
    mats = [rng.normal(0, 1, (4, 4)) for _ in range(200)]
    mats = [m + m.T for m in mats] + [sc.reference("kb8_63_formula_142")["hyps"][k]["N"].reshape(4, 4) for k in range(40)]
    for A in mats:
        w, v = np.linalg.eigh(A)
        if w[3] - w[2] < 1e-3 * abs(w[3]):
            continue
        q = np.array(ref.largest_eigenvector4(A.reshape(-1)), np.float64)
        e = v[:, 3] * (1 if v[0, 3] >= 0 else -1)
        assert q[0] >= 0 and np.abs(q - e).max() <= 1e-6, (A, q, e)
    # a tie takes the first of the largest diagonal entries; a diagonal matrix is left alone
    assert [float(x) for x in ref.largest_eigenvector4(np.diag([2.0, 5.0, 5.0, 1.0]).reshape(-1))] == [0.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize("key", sorted(sc.EXPECT))
def test_built_cases_end_as_built(key):
    want = sc.reference(key)
    assert (want["converged"], want["iterations"]) == sc.EXPECT[key], (key, want["hypothesis_inliers"])
    assert want["no_more"] == (not want["converged"])


@pytest.mark.parametrize("key", [k for k in RUN if sc.reference(k)["converged"]])
def test_converged_cases_recover_the_planted_transform_and_inliers(key):
    """(b) A hypothesis from three noise-free inliers reproduces the planted transform to float32 rounding amplified by the
    sample's geometry: points ~5 m from the camera carry 3e-7 m of rounding, a sample spans ~1 m, a thin triangle amplifies by up to
    ~100: 1e-4 on R and s - asserted at 2e-3, and t (a difference of terms of size |O1| ~ 6 m) at 2e-2 m.  identity poses keep the
    exact cases exact.  The inlier set is the planted one, and no pair is near its threshold under the winning hypothesis."""
    P, want = sc.CASES[key], sc.reference(key)
    s, R, t = P["truth"]
    if not P["fix_scale"] or s == 1.0:
        assert np.abs(want["R"].astype(np.float64) - R).max() <= 2e-3
        assert abs(float(want["s"]) / s - 1) <= 2e-3
        assert np.abs(want["t"].astype(np.float64) - t).max() <= 2e-2
    assert np.array_equal(want["inliers"].astype(bool), P["planted"]), key
    assert want["n_inliers"] == int(P["planted"].sum()) == want["n_best_inliers"]
    H = want["hyps"][want["best_iteration"] - 1]
    e1, e2 = ref.errors(P, want["G"], H)
    m1, m2 = np.array(want["G"]["max1"]), np.array(want["G"]["max2"])
    for e, m in ((e1, m1), (e2, m2)):
        assert not ((e > 0.5 * m) & (e < 2 * m)).any(), key  # no error within a factor 2 of its threshold
    inl = want["best_inliers"][P["pair_index"]].astype(bool)
    assert (e1[inl] < 1e-3 * m1[inl]).all() and (e2[inl] < 1e-3 * m2[inl]).all()
    assert (np.maximum(e1 / m1, e2 / m2)[~inl] > 50).all()


def test_every_case_agrees_with_the_literal_loop_of_iterate():
    """the selection applied to the counts after the fact is what the sequential loop (:218-294, chunks of 20) returns"""
    for key in sc.CASES:
        a, b = sc.reference(key), ref.solve_sequential(sc.CASES[key])
        for f in ("converged", "no_more", "iterations", "effective_iterations", "n_inliers", "n_best_inliers", "best_iteration"):
            assert a[f] == b[f], (key, f, a[f], b[f])
        for f in ("T12", "R", "t", "inliers", "best_inliers"):
            assert np.array_equal(np.asarray(a[f]).view(np.uint8), np.asarray(b[f]).view(np.uint8)), (key, f)
        assert np.array_equal(a["hypothesis_inliers"][:a["iterations"]], b["hypothesis_inliers"]), key


def test_cases_cover_what_they_are_for():
    r = {k: sc.reference(k) for k in sc.CASES}
    assert sorted({len(r[k]["G"]["idx"]) for k in RUN} & {3, 4, 63, 64, 65, 257}) == [3, 4, 63, 64, 65, 257]
    assert {r[k]["effective_iterations"] for k in RUN} >= {1, 2, 5, 35, 142, 300}
    assert all(r[k]["iterations"] == 0 and r[k]["no_more"] and not r[k]["inliers"].any() and np.array_equal(r[k]["T12"], np.eye(4)) for k in sc.JOBLESS)
    # the tie: several iterations hold the best count of a run that does not converge, and the last of them is the best
    t = r["n257_300_never_tie"]
    ties = np.nonzero(t["hypothesis_inliers"] == t["n_best_inliers"])[0]
    assert len(ties) >= 2 and t["best_iteration"] == ties[-1] + 1 and t["n_best_inliers"] == 60 and not t["inliers"].any()
    a, b = t["hyps"][ties[0]], t["hyps"][ties[-1]]
    assert not np.array_equal(a["T12"], b["T12"]) and np.array_equal(t["T12"][:3].reshape(-1), b["T12"])
    # three coincident points: NaN scale, no inlier; two coincident and three collinear points: finite, and evaluated
    d = r["n65_degenerate_then_last"]
    assert np.isnan(d["hyps"][0]["s"]) and d["hypothesis_inliers"][0] == 0
    assert np.isfinite(d["hyps"][1]["s"]) and np.isfinite(d["hyps"][2]["s"])
    # vec.norm() == 0 with theta = 0; the small-angle branch with a vector that is not 0; a rotation of nearly pi
    assert r["identity_exact"]["hyps"][0]["zero_vec"] and r["identity_exact"]["hyps"][0]["small_angle"]
    assert np.array_equal(r["identity_exact"]["T12"], np.eye(4, dtype=np.float32))
    assert r["rot0_scaled"]["hyps"][0]["small_angle"] and not r["rot0_scaled"]["hyps"][0]["zero_vec"]
    assert abs(np.trace(r["rot_pi"]["R"]) + 1) < 1e-2 and not r["rot_pi"]["hyps"][0]["small_angle"]
    s = sc.CASES["sparse_100_of_2000"]
    assert s["valid"].sum() == 100 and len(s["valid"]) == 2000 and not r["sparse_100_of_2000"]["best_inliers"][s["valid"] == 0].any()
    assert {(sc.CASES[k]["cam_model1"], sc.CASES[k]["cam_model2"]) for k in RUN} >= {(0, 0), (1, 1), (0, 1), (1, 0)}


def test_iteration_count_formula():
    """(c) SetRansacParameters by hand: ceil(log(1 - p) / log(1 - eps^3)) with eps = (float)minInliers / N"""
    ei = ref.effective_iterations
    assert ei(0.99, 3, 3, 300) == 1 and ei(0.99, 20, 20, 300) == 1                # minInliers == N
    assert ei(0.99, 2, 4, 300) == 35                                               # eps 0.5: log(0.01) / log(0.875) = 34.49
    assert ei(0.99, 15, 30, 300) == 35 and ei(0.99, 15, 30, 20) == 20              # the same ratio; clamped by maxIts
    assert ei(0.99, 20, 63, 300) == 142                                            # eps 0.31746: 4.60517 / 0.032520 = 141.6
    assert ei(0.99, 3, 4, 300) == 9                                                # eps 0.75: 4.60517 / 0.54818 = 8.40
    assert ei(0.5, 9, 10, 300) == 1                                                # log(0.5) / log(0.271) = 0.53 -> 1
    assert ei(0.99, 1, 60000, 300) == 300 and ei(0.99, 1, 60000, 1024) == 1024    # eps^3 = 4.6e-15: 9.9e14 iterations, beyond int
    assert ei(0.99, 1, 65535, 7) == 7
    assert ei(0.99, 0, 10, 300) == 300                                             # eps 0: log(1) = 0, the quotient is infinite
    assert ei(0.99, 0, 10, 1) == 1
    for n_min, n, p, m in ((15, 100, 0.99, 300), (40, 100, 0.9, 1000), (7, 9, 0.999, 50)):
        eps = float(np.float32(n_min) / np.float32(n))
        assert ei(p, n_min, n, m) == max(1, min(math.ceil(math.log(1 - p) / math.log(1 - eps ** 3)), m))


def test_draw_reduction_and_removal_against_the_literal_transcription():
    """(d) the closed form of the three indices is the list manipulation of :172-186, and never picks a pair twice"""
    rng = np.random.default_rng(11)
    for N in (3, 4, 5, 6, 7, 63, 64, 65, 257, 65535):
        reps = 4000 if N > 7 else 20000
        D = rng.integers(0, 2 ** 31, (reps, 3))
        D[:50] = rng.choice([0, 1, 2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30], (50, 3))  # the ends of the range
        for d in D:
            got = ref.sample(d, N)
            assert got == ref.sample_literal(d, N) and len(set(got)) == 3 and all(0 <= g < N for g in got), (N, d, got)
    for N in (3, 4, 5):  # every position triple of a small list
        for r0 in range(N):
            for r1 in range(N - 1):
                for r2 in range(N - 2):
                    d = [int((r0 + 0.5) * 2 ** 31 / N), int((r1 + 0.5) * 2 ** 31 / (N - 1)), int((r2 + 0.5) * 2 ** 31 / (N - 2))]
                    assert ref.sample(d, N) == ref.sample_literal(d, N)
    assert ref.random_int(2 ** 31 - 1, 65535) == 65534 and ref.random_int(0, 3) == 0

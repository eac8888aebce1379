"""Problems for the tests of ft_sim3_solver (Sim3Solver, reference src/Sim3Solver.cc): two keyframes with known poses, a known
Sim3 S12 = (s, R, t) between their camera frames (X1c = s R X2c + t), pairs of map points that obey it exactly (planted inliers,
observed without noise: what float32 storage leaves is ~1e-7 relative) and gross outliers whose camera-1 point is displaced
sideways by 1.2 - 2 times its depth, so that the error of an outlier under the true transform is at least 100 x its threshold
(asserted here, in float64, for every problem).  A problem is the dict of tests/sim3_solver_ref.py plus the truth; to_device()
turns it into the library's object.

The draws are random rand() values, except where a case needs a particular sample at a particular iteration: `samples` maps an
iteration to three pair indices (or "in" / "out": a random sample of three inliers / one that holds an outlier), and draws_for
builds the rand() values that DUtils::Random::RandomInt turns into exactly that sample.
"""
import functools

import numpy as np

from tests import sim3_solver_ref as ref
from tests.pose_opt_cases import KB8_CAM, KB8_CAM2, PINHOLE_CAM, _project64, _quat, _rodrigues

f32 = np.float32
CAMS = {"pinhole": (0, PINHOLE_CAM), "kb8": (1, KB8_CAM), "kb8b": (1, KB8_CAM2)}


def draws_for(sample, N):
    """three rand() values that pick the pair indices `sample` (:172-186): the middle of the interval RandomInt maps onto a position"""
    avail = list(range(N))
    out = []
    for i in sample:
        pos = avail.index(i)
        out.append(int((pos + 0.5) * 2 ** 31 / len(avail)))
        avail[pos] = avail[-1]
        avail.pop()
    assert ref.sample(out, N) == tuple(sample)
    return out


@functools.lru_cache(maxsize=None)
def problem(seed, N, n_in, n=None, cams=("pinhole", "pinhole"), fix_scale=False, scale=1.0, rotvec=(0.05, -0.1, 0.08), trans=(0.3, -0.2, 0.15),
            min_inliers=3, max_iterations=300, probability=0.99, samples=(), fill=None, special=None, identity_poses=False):
    """-> problem dict with N pairs among n entries (N by default), the first n_in pair slots of a seeded permutation planted
    inliers.  special: "degenerate" makes the pairs 0, 1, 2 one and the same point and the pairs 3, 4, 5 collinear (all inliers).
    samples: ((iteration, sample), ...); fill: "out" / "in" for every other iteration, None = random draws.
    Extra keys: truth = (s, R, t) float64, planted [n] bool (the planted inliers), pair_index [N]"""
    rng = np.random.default_rng(seed)
    n = N if n is None else n
    R, t, s = _rodrigues(np.asarray(rotvec, np.float64)), np.asarray(trans, np.float64), float(scale)
    z = rng.uniform(2.0, 6.0, N)
    X2 = np.stack([rng.uniform(-0.4, 0.4, N) * z, rng.uniform(-0.3, 0.3, N) * z, z], 1)
    inl = np.zeros(N, bool)
    inl[rng.permutation(N)[:n_in]] = True
    if special == "degenerate":
        inl[:6] = True
        X2[1] = X2[2] = X2[0]
        d = np.array([0.3, -0.2, 0.25])
        X2[4], X2[5] = X2[3] + d, X2[3] + 2.5 * d
    X1 = s * X2 @ R.T + t
    ang = rng.uniform(0, 2 * np.pi, N)
    off = np.stack([np.cos(ang), np.sin(ang), np.zeros(N)], 1) * (X1[:, 2] * rng.uniform(1.2, 2.0, N))[:, None]
    X1 = np.where(inl[:, None], X1, X1 + off)
    assert (X1[:, 2] > 0.5).all() and (X2[:, 2] > 0.5).all()
    if identity_poses:
        q1 = q2 = np.array([0, 0, 0, 1], f32)
        t1 = t2 = np.zeros(3, f32)
        W1, W2 = X1, X2
    else:
        R1, R2 = _rodrigues(rng.normal(0, 0.3, 3)), _rodrigues(rng.normal(0, 0.3, 3))
        c1, c2 = rng.normal(0, 1.0, 3), rng.normal(0, 1.0, 3)
        q1, q2 = _quat(R1).astype(f32), _quat(R2).astype(f32)
        q1, q2 = (q1 / f32(np.linalg.norm(q1.astype(np.float64)))).astype(f32), (q2 / f32(np.linalg.norm(q2.astype(np.float64)))).astype(f32)
        t1, t2 = c1.astype(f32), c2.astype(f32)
        W1, W2 = (X1 - c1) @ R1, (X2 - c2) @ R2  # Rcw^T (Xc - tcw)
    idx = np.sort(rng.permutation(n)[:N])
    valid = np.zeros(n, np.uint8)
    valid[idx] = 1
    wp1, wp2 = np.full((n, 3), 1e30, f32), np.full((n, 3), -1e30, f32)  # entries without a pair must never be read
    wp1[idx], wp2[idx] = W1.astype(f32), W2.astype(f32)
    sg1, sg2 = np.full(n, 1e-30, f32), np.full(n, 1e-30, f32)
    sg1[idx] = (f32(1.2) ** (2 * rng.integers(0, 4, N))).astype(f32)
    sg2[idx] = (f32(1.2) ** (2 * rng.integers(0, 4, N))).astype(f32)
    (m1, cam1), (m2, cam2) = CAMS[cams[0]], CAMS[cams[1]]
    # an outlier's error under the true transform, in float64: at least 100 x its threshold on one side
    Xt1, Xt2 = s * X2 @ R.T + t, (X1 - t) @ R / s
    e1 = ((_project64(m1, cam1, X1) - _project64(m1, cam1, Xt1)) ** 2).sum(1) / (9.210 * sg1[idx])
    e2 = ((_project64(m2, cam2, X2) - _project64(m2, cam2, Xt2)) ** 2).sum(1) / (9.210 * sg2[idx])
    assert (np.maximum(e1, e2)[~inl] >= 100).all() and (np.maximum(e1, e2)[inl] < 1e-6).all(), (seed, N)
    draws = rng.integers(0, 2 ** 31, 3 * max_iterations).astype(np.int64)
    ins, outs = np.nonzero(inl)[0], np.nonzero(~inl)[0]

    def pick(kind):
        if kind == "in":
            return tuple(int(v) for v in rng.choice(ins, 3, replace=False))
        o = int(rng.choice(outs))
        rest = rng.choice(np.setdiff1d(np.arange(N), [o]), 2, replace=False)
        return tuple(int(v) for v in rng.permutation([o, int(rest[0]), int(rest[1])]))

    chosen = dict(samples)
    for it in range(max_iterations):
        smp = chosen.get(it, fill)
        if smp is None:
            continue
        if isinstance(smp, str):
            smp = pick(smp)
        draws[3 * it:3 * it + 3] = draws_for(smp, N)
    planted = np.zeros(n, bool)
    planted[idx[inl]] = True
    return dict(valid=valid, world_pos1=wp1, world_pos2=wp2, sigma2_1=sg1, sigma2_2=sg2, Tcw1=(q1, t1), Tcw2=(q2, t2), cam_model1=m1,
                cam1=np.asarray(cam1, f32), cam_model2=m2, cam2=np.asarray(cam2, f32), fix_scale=bool(fix_scale), probability=probability,
                min_inliers=min_inliers, max_iterations=max_iterations, rand_draws=draws.astype(np.int32), truth=(s, R, t), planted=planted,
                pair_index=idx)


@functools.lru_cache(maxsize=None)
def reference(key):
    """the restatement's result of a committed case, computed once"""
    return ref.sim3_solver(CASES[key])


def to_device(orb, P, pinned=None):
    return orb.Sim3Problem(P["valid"], P["world_pos1"], P["world_pos2"], P["sigma2_1"], P["sigma2_2"], P["Tcw1"], P["Tcw2"], P["cam_model1"],
                           P["cam1"], P["cam_model2"], P["cam2"], P["fix_scale"], P["probability"], P["min_inliers"], P["max_iterations"],
                           P["rand_draws"], pinned=pinned)


# The committed cases.  Pair counts around the 64 lanes of a wave (63, 64, 65), the smallest (3, 4) and 257 (five steps of a
# wave, two of the selection's 256 threads); effective iteration counts 1, 2, 5 (not a multiple of the four iterations a workgroup
# of k_sim3_count takes), 9 and 142 (set by the formula, not by max_iterations) and 300; convergence at the first iteration, at the
# last, in between and never; every pairing of camera models; fix_scale with a true scale of 1, a free scale with 0.6 - 1.7.
# EXPECT: key -> (converged, iterations) where the case is built to end in a known way (test_sim3_solver_cpu.py asserts it).
CASES = {
    # N == min_inliers: one iteration, whose count N is not > min_inliers
    "n3_one_iteration": problem(1, 3, 3, min_inliers=3, max_iterations=300, scale=1.3),
    # the only sample there is: converges at iteration 1 of 5
    "n3_converges_first": problem(2, 3, 3, min_inliers=2, max_iterations=5, scale=0.8),
    "n4_formula_35": problem(3, 4, 3, min_inliers=2, max_iterations=300, scale=1.2),
    "kb8_63_formula_142": problem(4, 63, 40, cams=("kb8", "kb8b"), min_inliers=20, max_iterations=300, scale=1.7, samples=((0, "out"), (1, "out"))),
    "mixed_64_two_fixscale": problem(5, 64, 40, cams=("pinhole", "kb8"), fix_scale=True, min_inliers=10, max_iterations=2, samples=((0, "out"), (1, "in"))),
    # iterations 1 - 3: three coincident points (NaN scale), two coincident points, three collinear points; 4: an outlier; 5: inliers
    "n65_degenerate_then_last": problem(6, 65, 40, min_inliers=20, max_iterations=5, scale=0.6, special="degenerate",
                                        samples=((0, (0, 1, 2)), (1, (0, 1, 7)), (2, (3, 4, 5)), (3, "out"), (4, "in"))),
    # never converges (the inliers are not MORE than min_inliers); several all-inlier samples tie at 60, the last of them is the best
    "n257_300_never_tie": problem(7, 257, 60, min_inliers=60, max_iterations=300, scale=1.4, samples=((7, "in"), (200, "in"))),
    "sparse_100_of_2000": problem(8, 100, 70, n=2000, cams=("kb8", "pinhole"), min_inliers=15, max_iterations=40, scale=0.9, samples=((0, "out"),)),
    "jobless_5": problem(9, 5, 5, n=9, min_inliers=8, max_iterations=300),
    "jobless_empty": problem(10, 0, 0, n=0, min_inliers=1, max_iterations=3),
    # a rotation by pi - 1e-3 about the optical axis: q0 ~ 5e-4
    "rot_pi": problem(11, 20, 14, min_inliers=8, max_iterations=5, scale=1.1, rotvec=(0.0, 0.0, np.pi - 1e-3), samples=((0, "in"),)),
    # both keyframes at the origin, the same points on both sides: N's first row is exactly 0 off the diagonal, the eigenvector is
    # exactly (1, 0, 0, 0): vec.norm() == 0 and the small-angle branch of SO3::exp with theta = 0
    "identity_exact": problem(12, 20, 14, fix_scale=True, min_inliers=8, max_iterations=5, rotvec=(0.0, 0.0, 0.0), trans=(0.0, 0.0, 0.0),
                              identity_poses=True, samples=((0, "in"),)),
    # no rotation, a scale and a translation: an angle of ~1e-7, the small-angle branch with vec.norm() != 0
    "rot0_scaled": problem(13, 20, 14, min_inliers=8, max_iterations=5, scale=1.5, rotvec=(0.0, 0.0, 0.0), identity_poses=True,
                           samples=((0, "in"),)),
}
EXPECT = {"n3_one_iteration": (False, 1), "n3_converges_first": (True, 1), "mixed_64_two_fixscale": (True, 2), "n65_degenerate_then_last": (True, 5),
          "n257_300_never_tie": (False, 300), "rot_pi": (True, 1), "identity_exact": (True, 1), "rot0_scaled": (True, 1)}
JOBLESS = ["jobless_5", "jobless_empty"]
# batches of mixed sizes and models (GPU tests): one problem, only jobless problems, jobless problems in the middle
BATCHES = {"one": ["kb8_63_formula_142"], "only_jobless": ["jobless_5", "jobless_empty", "jobless_5"],
           "jobless_in_the_middle": ["n4_formula_35", "jobless_5", "mixed_64_two_fixscale", "jobless_empty", "n3_converges_first", "rot_pi"]}

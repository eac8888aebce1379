"""Sim3Solver (reference src/Sim3Solver.cc) restated in Python, statement by statement, driven as its only call site drives it
(src/LoopClosing.cc:698-710): SetRansacParameters(p, minInliers, maxIts), then iterate(20, ...) until bConverge || bNoMore.

The checker of ft_sim3_solver.  All float arithmetic is numpy float32 scalars, every operation rounded on its own, in the
reference's order; three-term sums (dot, norm, a coefficient of a small product, rowwise().sum()) associate as e0 + (e1 + e2)
(Eigen's redux_novec_unroller, as everywhere in these restatements); sqrtf, atan2f, sinf, cosf are the host's glibc, and
pCamera->project is reloc_search_ref's.  What is NOT the reference's, and is the same text as kernels_sim3_solver.hip:
  - the eigenvector of N's largest eigenvalue: a cyclic two-sided Jacobi in float64 (largest_eigenvector4) where the reference
    runs Eigen::EigenSolver<Matrix4f>; sign normalised to q0 >= 0;
  - nom / den of the scale: nine float terms added one after the other in column-major order;
  - the iteration count: min(nIterations, maxIts) taken in double, an infinite or NaN quotient counting as more than maxIts;
  - every effective iteration is evaluated and consumes three draws; the sequential selection is applied to the counts after
    the fact (select) - `solve_sequential` is the literal loop of iterate and must agree (test_sim3_solver_cpu.py).
A problem is a dict: valid [n], world_pos1 / world_pos2 [n, 3], sigma2_1 / sigma2_2 [n], Tcw1 / Tcw2 = (q xyzw, t), cam_model1,
cam1 [8], cam_model2, cam2 [8], fix_scale, probability, min_inliers, max_iterations, rand_draws [3 * max_iterations]."""
import math

import numpy as np

from tests.reloc_search_ref import _m, project

f32 = np.float32
f64 = np.float64
RAND_MAX = 2147483647


def sum3(e0, e1, e2):
    """e0 + (e1 + e2)"""
    return f32(e0 + f32(e1 + e2))


def dot3(a, b):
    return sum3(f32(a[0] * b[0]), f32(a[1] * b[1]), f32(a[2] * b[2]))


def quat_matrix(w, x, y, z):
    """Quaternionf(w, x, y, z).toRotationMatrix(), row-major [9]"""
    tx, ty, tz = f32(f32(2) * x), f32(f32(2) * y), f32(f32(2) * z)
    twx, twy, twz = f32(tx * w), f32(ty * w), f32(tz * w)
    txx, txy, txz = f32(tx * x), f32(ty * x), f32(tz * x)
    tyy, tyz, tzz = f32(ty * y), f32(tz * y), f32(tz * z)
    one = f32(1)
    return [f32(one - f32(tyy + tzz)), f32(txy - twz), f32(txz + twy),
            f32(txy + twz), f32(one - f32(txx + tzz)), f32(tyz - twx),
            f32(txz - twy), f32(tyz + twx), f32(one - f32(txx + tyy))]


def largest_eigenvector4(N):
    """Eigenvector of the largest eigenvalue of the symmetric 4 x 4 N (float64, row-major [16]), the first on a tie, q[0] >= 0,
    narrowed to float32.  Cyclic two-sided Jacobi: pivots (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) per sweep; a pivot is rotated away
    unless it is 0 or not above 1e-18 (|app| + |aqq|); the sweeps end with the first that rotates nothing, or after 30."""
    A = [f64(v) for v in N]
    V = [f64(1.0 if i % 5 == 0 else 0.0) for i in range(16)]
    one = f64(1.0)
    for _ in range(30):
        rotated = False
        for p in range(3):
            for r in range(p + 1, 4):
                apq, app, aqq = A[4 * p + r], A[5 * p], A[5 * r]
                if apq == 0.0 or not (abs(apq) > f64(1e-18) * (abs(app) + abs(aqq))):
                    continue
                rotated = True
                theta = (aqq - app) / (f64(2.0) * apq)
                t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                A[5 * p] = app - t * apq
                A[5 * r] = aqq + t * apq
                A[4 * p + r] = A[4 * r + p] = f64(0.0)
                for k in range(4):
                    if k != p and k != r:
                        akp, akq = A[4 * k + p], A[4 * k + r]
                        A[4 * k + p] = A[4 * p + k] = c * akp - s * akq
                        A[4 * k + r] = A[4 * r + k] = s * akp + c * akq
                    vkp, vkq = V[4 * k + p], V[4 * k + r]
                    V[4 * k + p] = c * vkp - s * vkq
                    V[4 * k + r] = s * vkp + c * vkq
        if not rotated:
            break
    best, top = 0, A[0]
    for j in range(1, 4):
        if A[5 * j] > top:
            top, best = A[5 * j], j
    v = [V[4 * i + best] for i in range(4)]
    if v[0] < 0:
        v = [-e for e in v]
    return [f32(e) for e in v]


def random_int(r, d):
    """DUtils::Random::RandomInt(0, d - 1) of the draw r"""
    return int(f64(r) / f64(2147483648.0) * f64(d))


def sample(draws, N):
    """the three pair indices of :172-186 in closed form (vAvailableIndices = 0 .. N - 1, swap-with-back removal)"""
    r0, r1, r2 = random_int(draws[0], N), random_int(draws[1], N - 1), random_int(draws[2], N - 2)
    back1 = N - 1 if N - 2 == r0 else N - 2
    return r0, (N - 1 if r1 == r0 else r1), (back1 if r2 == r1 else (N - 1 if r2 == r0 else r2))


def sample_literal(draws, N):
    """:172-186 as written: a fresh copy of mvAllIndices per iteration"""
    avail = list(range(N))
    out = []
    for i in range(3):
        randi = random_int(draws[i], len(avail))
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return tuple(out)


def effective_iterations(probability, min_inliers, N, max_its):
    """mRansacMaxIts of SetRansacParameters (:123-147), the min taken in double"""
    if min_inliers == N:
        return 1
    eps = f32(f32(min_inliers) / f32(N))
    den = math.log(1.0 - math.pow(float(eps), 3.0))
    num = math.log(1.0 - probability)
    q = num / den if den != 0.0 else math.inf  # IEEE division by zero (Python raises): infinite of either sign, or NaN - all "more than max_its"
    n = int(math.ceil(q)) if (math.isfinite(q) and math.ceil(q) < max_its) else max_its
    return max(1, n)


def centroid(P):
    """ComputeCentroid: P = three points (columns) -> Pr, C"""
    C = [f32(sum3(P[0][k], P[1][k], P[2][k]) / f32(3)) for k in range(3)]
    return [[f32(P[i][k] - C[k]) for k in range(3)] for i in range(3)], C


def compute_sim3(P1, P2, fix_scale):
    """ComputeSim3 (:311-414) -> dict(T12 [12] rows [sR | t], T21 [12], R [9], s, N [16] float64: the matrix handed to the solver,
    zero_vec: vec.norm() == 0, small_angle: the small-angle branch of SO3::exp was taken)"""
    with np.errstate(all="ignore"):
        Pr1, O1 = centroid(P1)
        Pr2, O2 = centroid(P2)
        M = [[sum3(f32(Pr2[0][i] * Pr1[0][j]), f32(Pr2[1][i] * Pr1[1][j]), f32(Pr2[2][i] * Pr1[2][j])) for j in range(3)] for i in range(3)]
        N11 = f32(f32(M[0][0] + M[1][1]) + M[2][2])
        N12 = f32(M[1][2] - M[2][1])
        N13 = f32(M[2][0] - M[0][2])
        N14 = f32(M[0][1] - M[1][0])
        N22 = f32(f32(M[0][0] - M[1][1]) - M[2][2])
        N23 = f32(M[0][1] + M[1][0])
        N24 = f32(M[2][0] + M[0][2])
        N33 = f32(f32(-M[0][0] + M[1][1]) - M[2][2])
        N34 = f32(M[1][2] + M[2][1])
        N44 = f32(f32(-M[0][0] - M[1][1]) + M[2][2])
        Nd = [f64(v) for v in (N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44)]
        q = largest_eigenvector4(Nd)
        vec = [q[1], q[2], q[3]]
        nv = _m("sqrtf", dot3(vec, vec))
        ang = _m("atan2f", nv, q[0])
        if nv != 0:
            k = f32(f32(2) * ang)
            vec = [f32(f32(k * v) / nv) for v in vec]
        theta_sq = dot3(vec, vec)
        small = bool(theta_sq < f32(f32(1e-5) * f32(1e-5)))
        if small:
            po4 = f32(theta_sq * theta_sq)
            imag = f32(f32(f32(0.5) - f32(f32(1.0 / 48.0) * theta_sq)) + f32(f32(1.0 / 3840.0) * po4))
            real = f32(f32(f32(1) - f32(f32(1.0 / 8.0) * theta_sq)) + f32(f32(1.0 / 384.0) * po4))
        else:
            theta = _m("sqrtf", theta_sq)
            half = f32(f32(0.5) * theta)
            imag = f32(_m("sinf", half) / theta)
            real = _m("cosf", half)
        R = quat_matrix(real, f32(imag * vec[0]), f32(imag * vec[1]), f32(imag * vec[2]))
        P3 = [[dot3(R[3 * k:3 * k + 3], Pr2[i]) for k in range(3)] for i in range(3)]
        s = f32(1.0)
        if not fix_scale:
            nom = den = None
            for i in range(3):
                for k in range(3):
                    a, b = f32(Pr1[i][k] * P3[i][k]), f32(P3[i][k] * P3[i][k])
                    nom = a if nom is None else f32(nom + a)
                    den = b if den is None else f32(den + b)
            s = f32(f64(nom) / f64(den))
        sR = [f32(s * r) for r in R]
        t = [f32(O1[i] - dot3(sR[3 * i:3 * i + 3], O2)) for i in range(3)]
        inv = f32(f64(1.0) / f64(s))
        T12, T21 = [f32(0)] * 12, [f32(0)] * 12
        for i in range(3):
            row = [f32(inv * R[3 * j + i]) for j in range(3)]
            for j in range(3):
                T21[4 * i + j] = row[j]
                T12[4 * i + j] = sR[3 * i + j]
            T12[4 * i + 3] = t[i]
            T21[4 * i + 3] = dot3([-v for v in row], t)
    return dict(T12=np.array(T12, f32), T21=np.array(T21, f32), R=np.array(R, f32), s=s, N=np.array(Nd, f64),
                zero_vec=bool(nv == 0), small_angle=small)


def rotation_of(q):
    """GetRotation() of a pose held as Sophus::SE3f"""
    q = [f32(v) for v in q]
    return quat_matrix(q[3], q[0], q[1], q[2])


def gather(P):
    """the constructor (:35-121) -> dict(idx = mvnIndices1, X1, X2 [N, 3], max1, max2 [N], P1, P2 [N, 2])"""
    R1, R2 = rotation_of(P["Tcw1"][0]), rotation_of(P["Tcw2"][0])
    t1, t2 = [f32(v) for v in P["Tcw1"][1]], [f32(v) for v in P["Tcw2"][1]]
    idx = [int(i) for i in np.nonzero(np.asarray(P["valid"]))[0]]
    X1, X2, m1, m2, p1, p2 = [], [], [], [], [], []
    for i in idx:
        w1, w2 = [f32(v) for v in P["world_pos1"][i]], [f32(v) for v in P["world_pos2"][i]]
        x1 = [f32(dot3(R1[3 * k:3 * k + 3], w1) + t1[k]) for k in range(3)]
        x2 = [f32(dot3(R2[3 * k:3 * k + 3], w2) + t2[k]) for k in range(3)]
        X1.append(x1), X2.append(x2)
        m1.append(f32(9.210 * float(f32(P["sigma2_1"][i]))))
        m2.append(f32(9.210 * float(f32(P["sigma2_2"][i]))))
        p1.append(project(P["cam_model1"], P["cam1"], x1))
        p2.append(project(P["cam_model2"], P["cam2"], x2))
    return dict(idx=idx, X1=X1, X2=X2, max1=m1, max2=m2, P1=p1, P2=p2)


def project_all(model, cam, A):
    """pCamera->project of the rows of A [N, 3] float32 -> u, v [N].  The pinhole form is elementwise float32 array arithmetic
    (numpy rounds every elementwise operation on its own, as the scalars do); KannalaBrandt8 needs glibc's functions per point."""
    if model == 0:
        cam = [f32(c) for c in cam]
        return (A[:, 0] * cam[0] / A[:, 2] + cam[2]).astype(f32), (A[:, 1] * cam[1] / A[:, 2] + cam[3]).astype(f32)
    uv = [project(model, cam, a) for a in A]
    return np.array([p[0] for p in uv], f32), np.array([p[1] for p in uv], f32)


def errors(P, G, H):
    """CheckInliers (:417-441) under the hypothesis H -> err1, err2 [N] float32"""
    T12, T21 = H["T12"], H["T21"]
    X1, X2 = np.array(G["X1"], f32).reshape(-1, 3), np.array(G["X2"], f32).reshape(-1, 3)
    P1, P2 = np.array(G["P1"], f32).reshape(-1, 2), np.array(G["P2"], f32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        # R X + t: a row of the product is e0 + (e1 + e2)
        a = np.stack([(T12[4 * k] * X2[:, 0] + (T12[4 * k + 1] * X2[:, 1] + T12[4 * k + 2] * X2[:, 2])) + T12[4 * k + 3] for k in range(3)], 1)
        b = np.stack([(T21[4 * k] * X1[:, 0] + (T21[4 * k + 1] * X1[:, 1] + T21[4 * k + 2] * X1[:, 2])) + T21[4 * k + 3] for k in range(3)], 1)
        assert a.dtype == f32 and b.dtype == f32
        u1x, u1y = project_all(P["cam_model1"], P["cam1"], a)
        u2x, u2y = project_all(P["cam_model2"], P["cam2"], b)
        d1x, d1y = P1[:, 0] - u1x, P1[:, 1] - u1y
        d2x, d2y = u2x - P2[:, 0], u2y - P2[:, 1]
        e1, e2 = d1x * d1x + d1y * d1y, d2x * d2x + d2y * d2y
    assert e1.dtype == f32 and e2.dtype == f32
    return e1, e2


def check_inliers(P, G, H):
    e1, e2 = errors(P, G, H)
    with np.errstate(invalid="ignore"):
        return (e1 < np.array(G["max1"], f32)) & (e2 < np.array(G["max2"], f32))


def hypothesis(P, G, it):
    """the sample and ComputeSim3 of iteration `it` (from 0)"""
    i = sample(P["rand_draws"][3 * it:3 * it + 3], len(G["idx"]))
    return compute_sim3([G["X1"][k] for k in i], [G["X2"][k] for k in i], P["fix_scale"]), i


def select(counts, min_inliers):
    """the sequential selection of iterate on the counts of every iteration -> (converged, stop, best): indices from 0"""
    stop = next((k for k, c in enumerate(counts) if c > min_inliers), None)
    converged = stop is not None
    last = stop if converged else len(counts) - 1
    top = max(counts[:last + 1])
    best = max(k for k in range(last + 1) if counts[k] == top)
    return converged, last, best


def _jobless(P):
    n = len(P["valid"])
    return dict(converged=False, no_more=True, iterations=0, effective_iterations=0, n_inliers=0, n_best_inliers=0, best_iteration=0,
                T12=np.eye(4, dtype=f32), R=np.eye(3, dtype=f32), t=np.zeros(3, f32), s=f32(1), inliers=np.zeros(n, np.uint8),
                best_inliers=np.zeros(n, np.uint8), hypothesis_inliers=np.zeros(0, np.int32))


def _result(P, G, H, flags, converged, iterations, eff, best, counts):
    n = len(P["valid"])
    scat = np.zeros(n, np.uint8)
    scat[np.array(G["idx"], int)] = flags.astype(np.uint8)
    T = np.eye(4, dtype=f32)
    T[:3, :] = H["T12"].reshape(3, 4)
    nb = int(flags.sum())
    return dict(converged=converged, no_more=not converged, iterations=iterations, effective_iterations=eff, n_inliers=nb if converged else 0,
                n_best_inliers=nb, best_iteration=best + 1, T12=T, R=H["R"].reshape(3, 3), t=T[:3, 3].copy(), s=H["s"],
                inliers=scat if converged else np.zeros(n, np.uint8), best_inliers=scat, hypothesis_inliers=np.array(counts, np.int32))


def sim3_solver(P):
    """what ft_sim3_solver returns for P: every effective iteration evaluated, the selection applied to the counts.  Extra keys:
    hyps (every hypothesis), G (the gathered pairs)"""
    G = gather(P)
    N = len(G["idx"])
    if N < P["min_inliers"]:
        return _jobless(P)
    assert N >= 3
    eff = effective_iterations(P["probability"], P["min_inliers"], N, P["max_iterations"])
    hyps = [hypothesis(P, G, it)[0] for it in range(eff)]
    flags = [check_inliers(P, G, H) for H in hyps]
    counts = [int(f.sum()) for f in flags]
    converged, last, best = select(counts, P["min_inliers"])
    out = _result(P, G, hyps[best], flags[best], converged, last + 1, eff, best, counts)
    out.update(hyps=hyps, G=G)
    return out


def solve_sequential(P):
    """iterate(20, ...) until bConverge || bNoMore, as written (:218-294): stops drawing at convergence.  Same keys without the
    counts behind the stop."""
    G = gather(P)
    N = len(G["idx"])
    if N < P["min_inliers"]:
        return _jobless(P)
    eff = effective_iterations(P["probability"], P["min_inliers"], N, P["max_iterations"])
    mn_iterations, best_n, best = 0, 0, None
    counts = []
    while True:  # the call site's loop
        cur = 0
        while mn_iterations < eff and cur < 20:
            cur += 1
            mn_iterations += 1
            H, _ = hypothesis(P, G, mn_iterations - 1)
            fl = check_inliers(P, G, H)
            ni = int(fl.sum())
            counts.append(ni)
            if ni >= best_n:
                best, best_n = (H, fl, mn_iterations - 1), ni
                if ni > P["min_inliers"]:
                    return _result(P, G, H, fl, True, mn_iterations, eff, mn_iterations - 1, counts)
        if mn_iterations >= eff:
            return _result(P, G, best[0], best[1], False, mn_iterations, eff, best[2], counts)

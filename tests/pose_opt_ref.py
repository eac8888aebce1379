"""Float64 numpy restatement of Optimizer::PoseOptimization(Frame*) (reference src/Optimizer.cc:814-1114) with the g2o pieces it
runs: the three unary edges (src/OptimizableTypes.cpp, Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp), the quadratic form of
base_unary_edge.hpp with the Huber kernel, Levenberg-Marquardt as optimization_algorithm_levenberg.cpp:61-194 runs it, a dense
6 x 6 LDLT, and SE3Quat::exp.  What ft_pose_optimization is tested against.

Operation for operation, every float narrowing in its place: the float delta and the float dsqr of the Huber kernel, the float invz
of the stereo edge, the float theta / psi of KannalaBrandt8::project (atan2f / sqrtf are the host's glibc through ctypes), camera
parameters as floats promoted to double, the float products 3 * k0 ... 9 * k3 of KannalaBrandt8::projectJac, the float chi2 of the
classification.  The arithmetic of an edge is vectorised over the edges (elementwise numpy is the scalar operation per element);
the SUMS over the edges - H, b and the robust chi2 - run sequentially in g2o's order, the order of the active edges, which is
keypoint order (np.cumsum accumulates left to right).  `order` permutes that summation and nothing else: POSE_TOL is measured with it.

Not pinned against a g2o binary: sums of three are taken left to right where Eigen may associate otherwise,
the LDLT does not pivot, pow(x, 3) is x * x * x, the solver's x starts at zero, and the double sin / cos / atan2 are the routines
written out below, not glibc's.

Inputs: a frame is a dict(N, nleft, has_point [N] uint8, world_pos [N, 3] f32, keys [nL] KP_DTYPE (mvKeysUn, or mvKeys of the left
camera), keys_right [N - nleft] or None, uright [N] f32 or None, inv_level_sigma2 [nlevels] f32, cam_model, cam [8] f32, cam2 [8] f32,
mbf, Tcw (q [4] xyzw, t [3]) f32, Trl likewise or None).
"""
import ctypes as C

import numpy as np

f32 = np.float32
f64 = np.float64

_libm = C.CDLL("libm.so.6")
for _n, _k in (("sqrtf", 1), ("atan2f", 2)):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float] * _k


def _atan2f(y, x):
    return np.array([_libm.atan2f(float(a), float(b)) for a, b in zip(y, x)], f32)


DELTA = (float(f32(np.sqrt(5.991))), float(f32(np.sqrt(7.815))))   # const float deltaMono = sqrt(5.991), deltaStereo (:852-853)
DSQR = tuple(float(f32(d * d)) for d in DELTA)                      # RobustKernelHuber::dsqr is a float (robust_kernel_impl.h:84)
TH = (f32(5.991), f32(7.815))                                       # const float chi2Mono[4], chi2Stereo[4] (:1001-1002)
DBL_MAX = np.finfo(f64).max
MONO, RIGHT, STEREO = 0, 1, 2
MAX_EDGES = 2000                                                    # FT_POSE_OPT_MAX_EDGES


# ---- sin / cos / atan2 of doubles -----------------------------------------------------------------------------------------------------
# The device's libm is not the host's, and a Levenberg-Marquardt run that has converged decides its last steps on the last bits of
# chi2.  So the three double routines the text calls are written out once - fdlibm's kernels (k_sin.c, k_cos.c, s_atan.c, e_atan2.c of
# FreeBSD msun / Sun's fdlibm) behind a two-term Cody-Waite reduction - and evaluated operation for operation by the kernel
# (kernels_pose_opt.hip) and here.  test_pose_opt_cpu.py holds them against numpy's (a few ulp).
_S = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06,
      -2.50507602534068634195e-08, 1.58969099521155010221e-10)
_CC = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07,
       2.08757232129817482790e-09, -1.13596475577881948265e-11)
_AT = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
       9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
       4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02)
_ATANHI = (4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00)
_ATANLO = (2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17)
_PI, _PI_LO = 3.1415926535897931160e+00, 1.2246467991473531772e-16


def sincos(x):
    """-> sin(x), cos(x)"""
    x = np.asarray(x, f64)
    with np.errstate(all="ignore"):
        k = np.rint(x * 6.36619772367581382433e-01)
        r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11
        z = r * r
        s = r + (r * z) * (_S[0] + z * (_S[1] + z * (_S[2] + z * (_S[3] + z * (_S[4] + z * _S[5])))))
        c = 1.0 - (0.5 * z - (z * z) * (_CC[0] + z * (_CC[1] + z * (_CC[2] + z * (_CC[3] + z * (_CC[4] + z * _CC[5]))))))
        n = np.where(np.isfinite(k), k, 0).astype(np.int64) & 3
    return np.where(n == 0, s, np.where(n == 1, c, np.where(n == 2, -s, -c))), np.where(n == 0, c, np.where(n == 1, -s, np.where(n == 2, -c, s)))


def _atan_pos(ax):
    """atan of ax >= 0"""
    with np.errstate(all="ignore"):
        idx = np.where(ax < 0.4375, -1, np.where(ax < 0.6875, 0, np.where(ax < 1.1875, 1, np.where(ax < 2.4375, 2, 3))))
        t = np.where(idx == -1, ax, np.where(idx == 0, (2.0 * ax - 1.0) / (2.0 + ax), np.where(idx == 1, (ax - 1.0) / (ax + 1.0),
                     np.where(idx == 2, (ax - 1.5) / (1.0 + 1.5 * ax), -1.0 / ax))))
        z = t * t
        w = z * z
        s1 = z * (_AT[0] + w * (_AT[2] + w * (_AT[4] + w * (_AT[6] + w * (_AT[8] + w * _AT[10])))))
        s2 = w * (_AT[1] + w * (_AT[3] + w * (_AT[5] + w * (_AT[7] + w * _AT[9]))))
        hi = np.where(idx == 0, _ATANHI[0], np.where(idx == 1, _ATANHI[1], np.where(idx == 2, _ATANHI[2], _ATANHI[3])))
        lo = np.where(idx == 0, _ATANLO[0], np.where(idx == 1, _ATANLO[1], np.where(idx == 2, _ATANLO[2], _ATANLO[3])))
        return np.where(idx == -1, t - t * (s1 + s2), hi - ((t * (s1 + s2) - lo) - t))


def atan2d(y, x):
    y, x = np.asarray(y, f64), np.asarray(x, f64)
    with np.errstate(all="ignore"):
        a = _atan_pos(np.abs(y / x))
        r = np.where(x == 0, np.where(y == 0, 0.0, 0.5 * _PI), np.where(x > 0, a, _PI - (a - _PI_LO)))
        return np.where(y < 0, -r, r)


# ---- SE3Quat (Thirdparty/g2o/g2o/types/se3quat.h) with Eigen's quaternion ---------------------------------------------------------
def _normalized(q):
    q = np.array(q, f64)
    if q[3] < 0:
        q = q * -1.0
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return q / n


def _rot(q, v):
    """Eigen's Quaternion * vector: uv = 2 vec x v; v + w uv + vec x uv.  v: [..., 3]"""
    x, y, z, w = q
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    ux, uy, uz = y * v2 - z * v1, z * v0 - x * v2, x * v1 - y * v0
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return np.stack([(v0 + w * ux) + (y * uz - z * uy), (v1 + w * uy) + (z * ux - x * uz), (v2 + w * uz) + (x * uy - y * ux)], -1)


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], f64)


def se3(q, t):
    return _normalized(q), np.array(t, f64)


def se3_mul(A, B):
    return _normalized(_qmul(A[0], B[0])), A[1] + _rot(A[0], B[1])


def _to_rot(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]], f64)


def _quat_of(R):
    t = (R[0, 0] + R[1, 1]) + R[2, 2]
    q = np.zeros(4, f64)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def _mat3(A, B):
    return np.array([[(A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j] for j in range(3)] for i in range(3)], f64)


def se3_exp(u):
    """SE3Quat::exp (se3quat.h:223-257): omega = u[0:3], upsilon = u[3:6]"""
    ox, oy, oz = u[0], u[1], u[2]
    theta = np.sqrt((ox * ox + oy * oy) + oz * oz)
    Om = np.array([[0.0, -oz, oy], [oz, 0.0, -ox], [-oy, ox, 0.0]], f64)
    Om2 = _mat3(Om, Om)
    I = np.eye(3)
    if theta < 0.00001:
        R = (I + Om) + Om2
        V = R
    else:
        sn, cs = (float(v) for v in sincos(theta))
        a = sn / theta
        b = (1.0 - cs) / (theta * theta)
        c = (theta - sn) / (theta * theta * theta)
        R = (I + a * Om) + b * Om2
        V = (I + b * Om) + c * Om2
    up = u[3:6]
    t = np.array([(V[i, 0] * up[0] + V[i, 1] * up[1]) + V[i, 2] * up[2] for i in range(3)], f64)
    return _normalized(_quat_of(R)), t


# ---- cameras ---------------------------------------------------------------------------------------------------------------------
def _project(model, cam, P):
    """pCamera->project(Vector3d): Pinhole.cpp:35, KannalaBrandt8.cpp:46-63.  cam: float64 copies of the float parameters"""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        if model == 0:
            return np.stack([cam[0] * x / z + cam[2], cam[1] * y / z + cam[3]], 1)
        r2 = x * x + y * y
        sq = np.array([_libm.sqrtf(float(v)) for v in r2.astype(f32)], f32)
        theta = _atan2f(sq, z.astype(f32)).astype(f64)
        psi = _atan2f(y.astype(f32), x.astype(f32)).astype(f64)
        t2 = theta * theta
        t3 = theta * t2
        t5 = t3 * t2
        t7 = t5 * t2
        t9 = t7 * t2
        r = theta + cam[4] * t3 + cam[5] * t5 + cam[6] * t7 + cam[7] * t9
        sn, cs = sincos(psi)
        return np.stack([cam[0] * r * cs + cam[2], cam[1] * r * sn + cam[3]], 1)


def _project_jac(model, cam, camf, P):
    """-> [n, 2, 3] (Pinhole.cpp:71-81, KannalaBrandt8.cpp:145-175); camf: the float parameters (3 * k0 is a float product)"""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    J = np.zeros((len(P), 2, 3), f64)
    with np.errstate(all="ignore"):
        if model == 0:
            J[:, 0, 0] = cam[0] / z
            J[:, 0, 2] = -cam[0] * x / (z * z)
            J[:, 1, 1] = cam[1] / z
            J[:, 1, 2] = -cam[1] * y / (z * z)
            return J
        x2, y2, z2 = x * x, y * y, z * z
        r2 = x2 + y2
        r = np.sqrt(r2)
        r3 = r2 * r
        th = atan2d(r, z)
        th2 = th * th
        th3 = th2 * th
        th4 = th2 * th2
        th5 = th4 * th
        th6 = th2 * th4
        th7 = th6 * th
        th8 = th4 * th4
        th9 = th8 * th
        f = th + th3 * cam[4] + th5 * cam[5] + th7 * cam[6] + th9 * cam[7]
        k3, k5, k7, k9 = (float(f32(m) * camf[i]) for m, i in ((3, 4), (5, 5), (7, 6), (9, 7)))
        fd = 1 + k3 * th2 + k5 * th4 + k7 * th6 + k9 * th8
        den = r2 * (r2 + z2)
        J[:, 0, 0] = cam[0] * (fd * z * x2 / den + f * y2 / r3)
        J[:, 1, 0] = cam[1] * (fd * z * y * x / den - f * y * x / r3)
        J[:, 0, 1] = cam[0] * (fd * z * y * x / den - f * y * x / r3)
        J[:, 1, 1] = cam[1] * (fd * z * y2 / den + f * x2 / r3)
        J[:, 0, 2] = -cam[0] * fd * x / (r2 + z2)
        J[:, 1, 2] = -cam[1] * fd * y / (r2 + z2)
        return J


# ---- the edges ---------------------------------------------------------------------------------------------------------------------
def build_edges(F):
    """:858-993 -> dict(idx, kind, X [n, 3], obs [n, 3], w [n]) in keypoint order"""
    N, nleft = int(F["N"]), int(F["nleft"])
    idx, kind, obs, w = [], [], [], []
    inv = np.asarray(F["inv_level_sigma2"], f32)
    for i in range(N):
        if not F["has_point"][i]:
            continue
        if nleft == -1:
            kp = F["keys"][i]
            ur = f32(-1) if F["uright"] is None else f32(F["uright"][i])
            if ur < 0:
                kind.append(MONO), obs.append((kp["x"], kp["y"], 0))
            else:
                kind.append(STEREO), obs.append((kp["x"], kp["y"], ur))
        elif i < nleft:
            kp = F["keys"][i]
            kind.append(MONO), obs.append((kp["x"], kp["y"], 0))
        else:
            kp = F["keys_right"][i - nleft]
            kind.append(RIGHT), obs.append((kp["x"], kp["y"], 0))
        idx.append(i)
        w.append(inv[int(kp["octave"])])
    n = len(idx)
    X = np.asarray(F["world_pos"], f32).reshape(-1, 3)[np.asarray(idx, int)].astype(f64) if n else np.zeros((0, 3))
    return dict(idx=np.asarray(idx, int), kind=np.asarray(kind, int), X=X, obs=np.asarray(obs, f32).astype(f64).reshape(n, 3),
                w=np.asarray(w, f32).astype(f64))


class _Frame:
    def __init__(self, F, E):
        self.model = int(F["cam_model"])
        self.camf = [np.asarray(F["cam"], f32), np.asarray(F["cam2"] if F.get("cam2") is not None else F["cam"], f32)]
        self.cam = [c.astype(f64) for c in self.camf]
        self.bf = float(f32(F["mbf"]))
        self.Trl = se3(*F["Trl"]) if F.get("Trl") is not None else se3([0, 0, 0, 1], [0, 0, 0])
        self.Rrl = _to_rot(self.Trl[0])
        self.E = E
        self.sel = [np.nonzero(E["kind"] == k)[0] for k in (MONO, RIGHT, STEREO)]

    def errors(self, est, which):
        """computeError of the edges `which` (indices) at the estimate -> e [n, 3] (third component 0 for the two mono edges)"""
        E = self.E
        e = np.zeros((len(which), 3), f64)
        kind = E["kind"][which]
        X, obs = E["X"][which], E["obs"][which]
        with np.errstate(all="ignore"):
            m = kind == MONO
            if m.any():
                e[m, :2] = obs[m, :2] - _project(self.model, self.cam[0], _rot(est[0], X[m]) + est[1])
            m = kind == RIGHT
            if m.any():
                T = se3_mul(self.Trl, est)  # (mTrl * v1->estimate()).map(Xw)
                e[m, :2] = obs[m, :2] - _project(self.model, self.cam[1], _rot(T[0], X[m]) + T[1])
            m = kind == STEREO
            if m.any():
                P = _rot(est[0], X[m]) + est[1]
                c = self.cam[0]
                invz = (1.0 / P[:, 2]).astype(f32).astype(f64)  # const float invz = 1.0f / trans_xyz[2]
                u = P[:, 0] * invz * c[0] + c[2]
                v = P[:, 1] * invz * c[1] + c[3]
                e[m] = obs[m] - np.stack([u, v, u - self.bf * invz], 1)
        return e

    def jacobians(self, est, which):
        """linearizeOplus -> A [n, 3, 6] (row 2 zero for the mono edges)"""
        E = self.E
        A = np.zeros((len(which), 3, 6), f64)
        kind = E["kind"][which]
        X = E["X"][which]

        def se3deriv(P):
            x, y, z = P[:, 0], P[:, 1], P[:, 2]
            S = np.zeros((len(P), 3, 6), f64)
            S[:, 0, 1], S[:, 0, 2], S[:, 0, 3] = z, -y, 1
            S[:, 1, 0], S[:, 1, 2], S[:, 1, 4] = -z, x, 1
            S[:, 2, 0], S[:, 2, 1], S[:, 2, 5] = y, -x, 1
            return S

        def mm(L, R):  # [n, a, 3] x [n, 3, b], the inner sum left to right
            return (L[:, :, 0, None] * R[:, None, 0, :] + L[:, :, 1, None] * R[:, None, 1, :]) + L[:, :, 2, None] * R[:, None, 2, :]

        with np.errstate(all="ignore"):
            m = kind == MONO
            if m.any():
                P = _rot(est[0], X[m]) + est[1]
                A[m, :2] = mm(-_project_jac(self.model, self.cam[0], self.camf[0], P), se3deriv(P))
            m = kind == RIGHT
            if m.any():
                Pl = _rot(est[0], X[m]) + est[1]
                Pr = _rot(self.Trl[0], Pl) + self.Trl[1]  # mTrl.map(T_lw.map(Xw))
                JR = mm(-_project_jac(self.model, self.cam[1], self.camf[1], Pr), np.broadcast_to(self.Rrl, (len(Pl), 3, 3)))
                A[m, :2] = mm(JR, se3deriv(Pl))
            m = kind == STEREO
            if m.any():
                P = _rot(est[0], X[m]) + est[1]
                fx, fy = self.cam[0][0], self.cam[0][1]
                x, y = P[:, 0], P[:, 1]
                invz = 1.0 / P[:, 2]
                invz_2 = invz * invz
                J = np.zeros((len(P), 3, 6), f64)
                J[:, 0, 0] = x * y * invz_2 * fx
                J[:, 0, 1] = -(1 + (x * x * invz_2)) * fx
                J[:, 0, 2] = y * invz * fx
                J[:, 0, 3] = -invz * fx
                J[:, 0, 5] = x * invz_2 * fx
                J[:, 1, 0] = (1 + y * y * invz_2) * fy
                J[:, 1, 1] = -x * y * invz_2 * fy
                J[:, 1, 2] = -x * invz * fy
                J[:, 1, 4] = -invz * fy
                J[:, 1, 5] = y * invz_2 * fy
                J[:, 2, 0] = J[:, 0, 0] - self.bf * y * invz_2
                J[:, 2, 1] = J[:, 0, 1] + self.bf * x * invz_2
                J[:, 2, 2] = J[:, 0, 2]
                J[:, 2, 3] = J[:, 0, 3]
                J[:, 2, 5] = J[:, 0, 5] - self.bf * invz_2
                A[m] = J
        return A


def _chi2(e, w, dim3):
    """_error.dot(information() * _error)"""
    c = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
    return np.where(dim3, c + e[:, 2] * (w * e[:, 2]), c)


def _huber(chi2, stereo):
    """RobustKernelHuber::robustify -> rho[0], rho[1]"""
    delta = np.where(stereo, DELTA[1], DELTA[0])
    dsqr = np.where(stereo, DSQR[1], DSQR[0])
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi2)
        inl = chi2 <= dsqr
        return np.where(inl, chi2, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)


def _seqsum(a, perm):
    """the sum over the edges, one after the other in the order perm (axis 0)"""
    return np.cumsum(a[perm], axis=0)[-1]


def ldlt_solve(H, b):
    """6 x 6 LDLT of the lower triangle, no pivoting -> (x, positive, smallest d).  A factor that is not > 0 fails"""
    L = np.zeros((6, 6), f64)
    d = np.zeros(6, f64)
    for j in range(6):
        s = H[j, j]
        for k in range(j):
            s = s - L[j, k] * (L[j, k] * d[k])
        d[j] = s
        if not s > 0:
            return None, False, s
        for i in range(j + 1, 6):
            s = H[i, j]
            for k in range(j):
                s = s - L[i, k] * (L[j, k] * d[k])
            L[i, j] = s / d[j]
    y = np.zeros(6, f64)
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i, k] * y[k]
        y[i] = s
    z = y / d
    x = np.zeros(6, f64)
    for i in range(5, -1, -1):
        s = z[i]
        for k in range(i + 1, 6):
            s = s - L[k, i] * x[k]
        x[i] = s
    return x, True, d.min()


_LOWER = [(i, j) for i in range(6) for j in range(i + 1)]


def pose_optimization(F, order="forward", seed=0):
    """-> dict(Tcw (q, t) float32, outlier [N] uint8 (a copy of F['outlier'] where has_point is 0), ret, trace [4] of (iterations,
    rejected, chi), edge_margin, lm_margin, flags: what the run went through)"""
    E = build_edges(F)
    n = len(E["idx"])
    outlier = np.array(F.get("outlier", np.zeros(F["N"], np.uint8)), np.uint8).copy()
    outlier[E["idx"]] = 0  # mvbOutlier[i] = false with every edge (:869 ...), also in front of `return 0`
    q_in, t_in = np.asarray(F["Tcw"][0], f32), np.asarray(F["Tcw"][1], f32)
    res = dict(Tcw=(q_in.copy(), t_in.copy()), outlier=outlier, ret=0, trace=[(0, 0, 0.0)] * 4, edge_margin=np.inf, lm_margin=np.inf,
               flags=set(), n_edges=n, decisions=[])
    if n < 3:
        res["flags"].add("lt3")
        return res
    assert n <= MAX_EDGES
    fr = _Frame(F, E)
    stereo = E["kind"] == STEREO
    w = E["w"]
    est0 = se3(q_in.astype(f64), t_in.astype(f64))
    level = np.zeros(n, int)
    err = np.zeros((n, 3), f64)  # _error of every edge: what the last computeError left
    robust = True
    rng = np.random.default_rng(seed)
    trace = []
    edge_margin = np.inf
    decisions = []  # (round, iteration, trial, which, relative distance to flipping) of every Levenberg-Marquardt decision
    flags = res["flags"]
    est = est0
    n_bad = 0
    for rnd in range(4):
        est = est0  # :1008-1009
        act = np.nonzero(level == 0)[0]
        perm = {"forward": np.arange(len(act)), "reversed": np.arange(len(act))[::-1]}.get(order)
        if perm is None:
            perm = rng.permutation(len(act))
        its = rej = 0
        cur = 0.0
        if len(act):
            st, wa = stereo[act], w[act]

            def robust_chi(e):
                c = _chi2(e, wa, st)
                return _seqsum(_huber(c, st)[0] if robust else c, perm)

            lam = ni = 0.0
            lm_bad = 0
            x = np.zeros(6, f64)
            for it in range(10):
                err[act] = fr.errors(est, act)
                cur = robust_chi(err[act])
                ini = cur
                # buildSystem: linearizeOplus + constructQuadraticForm of every active edge
                A = fr.jacobians(est, act)
                e = err[act]
                rho1 = _huber(_chi2(e, wa, st), st)[1] if robust else np.ones(len(act))
                D = np.where(st, 3, 2)
                Hc = np.zeros((len(act), 21), f64)
                for c, (i, j) in enumerate(_LOWER):
                    wr = rho1 * wa
                    s = (A[:, 0, i] * wr) * A[:, 0, j] + (A[:, 1, i] * wr) * A[:, 1, j]
                    Hc[:, c] = np.where(D == 3, s + (A[:, 2, i] * wr) * A[:, 2, j], s)
                bc = np.zeros((len(act), 6), f64)
                for j in range(6):
                    s = ((rho1 * A[:, 0, j]) * wa) * e[:, 0] + ((rho1 * A[:, 1, j]) * wa) * e[:, 1]
                    bc[:, j] = np.where(D == 3, s + ((rho1 * A[:, 2, j]) * wa) * e[:, 2], s)
                with np.errstate(all="ignore"):
                    Hs, b = _seqsum(Hc, perm), -_seqsum(bc, perm)
                H = np.zeros((6, 6), f64)
                for c, (i, j) in enumerate(_LOWER):
                    H[i, j] = Hs[c]
                if it == 0:
                    lam = 1e-5 * max(abs(H[j, j]) for j in range(6))
                    ni = 2.0
                    lm_bad = 0
                rho = 0.0
                qmax = 0
                backup = est
                while True:
                    Hl = H.copy()
                    for j in range(6):
                        Hl[j, j] = H[j, j] + lam
                    xs, ok2, dmin = ldlt_solve(Hl, b)
                    with np.errstate(all="ignore"):
                        decisions.append((rnd, it, qmax, "positive", abs(dmin) / max(abs(Hl[j, j]) for j in range(6))))
                    if ok2:
                        x = xs
                    est = se3_mul(se3_exp(x), est)
                    err[act] = fr.errors(est, act)
                    tmp = robust_chi(err[act])
                    if not ok2:
                        tmp = DBL_MAX
                        flags.add("not_positive")
                    with np.errstate(all="ignore"):
                        rho = cur - tmp
                        if ok2:
                            decisions.append((rnd, it, qmax, "rho", abs(rho) / max(abs(cur), abs(tmp))))
                        scale = 0.0
                        for j in range(6):
                            scale += x[j] * (lam * x[j] + b[j])
                        scale += 1e-3
                        rho /= scale
                    if rho > 0 and np.isfinite(tmp):
                        t = 2 * rho - 1
                        alpha = min(1.0 - t * t * t, 2.0 / 3.0)
                        lam *= max(1.0 / 3.0, alpha)
                        ni = 2.0
                        cur = tmp
                        stale = False
                    else:
                        lam *= ni
                        ni *= 2
                        est = backup  # pop() restores the vertex; the errors stay those of the rejected estimate
                        rej += 1
                        stale = True
                        flags.add("rejected")
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                its += 1
                if qmax == 10 or rho == 0:
                    flags.add("terminate")
                    break
                with np.errstate(all="ignore"):
                    lhs = (ini - cur) * 1e3
                    decisions.append((rnd, it, qmax, "nbad", abs(lhs - ini) / abs(ini)))
                if lhs < ini:
                    lm_bad += 1
                else:
                    lm_bad = 0
                if lm_bad >= 3:
                    flags.add("nbad_stop")
                    break
            if stale:
                flags.add("stale")
        trace.append((its, rej, float(cur)))
        # :1014-1100: an outlier's error is recomputed at the final estimate, an inlier's is what the last evaluation left
        was = np.nonzero(level == 1)[0]
        if len(was):
            err[was] = fr.errors(est, was)
        c32 = _chi2(err, w, stereo).astype(f32)
        th = np.where(stereo, TH[1], TH[0]).astype(f32)
        with np.errstate(all="ignore"):
            edge_margin = min(edge_margin, float(np.min(np.abs(c32.astype(f64) - th.astype(f64)) / th.astype(f64))))
        new = (c32 > th).astype(int)
        if ((level == 1) & (new == 0)).any():
            flags.add("readmitted")
        level = new
        n_bad = int(new.sum())
        if rnd == 2:
            robust = False
        if n < 10:
            flags.add("lt10")
            break
    while len(trace) < 4:
        trace.append((0, 0, 0.0))
    outlier[E["idx"]] = level.astype(np.uint8)
    q = est[0].astype(f32)  # Sophus::SE3<float>(rotation().cast<float>(), ...) normalises the float quaternion
    nq = f32(np.sqrt(f32(f32(f32(q[0] * q[0]) + f32(q[1] * q[1])) + f32(q[2] * q[2])) + f32(q[3] * q[3])))
    res.update(Tcw=((q / nq).astype(f32), est[1].astype(f32)), outlier=outlier, ret=n - n_bad, trace=trace, edge_margin=edge_margin,
               lm_margin=min([0.0 if np.isnan(d[4]) else d[4] for d in decisions], default=np.inf), decisions=decisions)  # 0 / 0: on the edge
    return res

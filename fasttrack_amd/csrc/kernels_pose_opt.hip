// HIP kernel of Optimizer::PoseOptimization(Frame*) (reference src/Optimizer.cc:814-1114) for gfx950 (wave64): motion-only bundle
// adjustment of every frame of a call in one launch - the four rounds, g2o's Levenberg-Marquardt inside each
// (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-194, sparse_optimizer.cpp:354-419), the outlier classification
// between them (:1014-1100) - without a host round trip.
//   k_pose_opt   blockIdx.x = frame (job), 256 threads.  A thread owns the edges e = tid, tid + 256, ...: it evaluates their
//                error (the three computeError of src/OptimizableTypes.h:41-73 and types_six_dof_expmap.cpp:339-346), their
//                Jacobian (OptimizableTypes.cpp:49-107, types_six_dof_expmap.cpp:375-404) and their term of the quadratic form
//                (base_unary_edge.hpp:43-72 with RobustKernelHuber, robust_kernel_impl.cpp:78-91), all in double.
//                THE SUMS over the edges - the 21 entries of the lower triangle of H, the 6 of b, the robust chi2 - are taken in
//                g2o's order, one active edge after the other in keypoint order: the threads put the terms of 256 edges into LDS,
//                lane j of the first wave adds column j of the block to its running sum, edge by edge.  A run that has converged
//                decides its last steps (rho > 0, the _nBad criterion) on the last bits of chi2; with the reference's summation
//                order those bits are the reference's, where a tree over the lanes would give others - and a frame's result does
//                not depend on how many threads or frames there are.  No atomics on floating-point data.
//                The 6 x 6 LDLT, SE3Quat::exp, the update and the Levenberg-Marquardt bookkeeping are done by every thread on
//                the same sums: every branch below the edge loops is uniform over the workgroup, nothing is broadcast.
//                Every loop bound is a constant of the algorithm (4 rounds, 10 iterations, 10 trials) or the edge count; a NaN
//                fails every comparison and so takes the reference's rejection path (rho > 0 is false: the trial is rejected;
//                rho < 0 is false: the trials end).
// Contraction is off (Makefile), so every expression is evaluated as written; tests/pose_opt_ref.py is the same text in numpy.
// sin / cos / atan2 of doubles are written out here (fdlibm's kernels) as they are there: the device's libm is not the host's.
#include "ft_internal.h"
#include "ft_search.h"
#include "libm_f32.h"

namespace {

#define FT_POSE_T 256
#define FT_POSE_TERMS 28    // chi2, H (21, lower triangle row by row), b (6)
#define FT_POSE_PITCH 29    // doubles per edge in LDS: odd, so that the 28 lanes that add and the 256 that write spread over the banks

struct Se3d {
    double q[4], t[3];  // q: x y z w
};

// ---- sin, cos, atan2 (k_sin.c, k_cos.c, s_atan.c, e_atan2.c of fdlibm behind a two-term Cody-Waite reduction) -------------------
__device__ __forceinline__ void sincos_d(double x, double &sn, double &cs) {
    const double k = rint(x * 6.36619772367581382433e-01);
    const double r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11;
    const double z = r * r;
    const double s = r + (r * z) * (-1.66666666666666324348e-01 +
                                    z * (8.33333333332248946124e-03 +
                                         z * (-1.98412698298579493134e-04 +
                                              z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))));
    const double c = 1.0 - (0.5 * z - (z * z) * (4.16666666666666019037e-02 +
                                                 z * (-1.38888888888741095749e-03 +
                                                      z * (2.48015872894767294178e-05 +
                                                           z * (-2.75573143513906633035e-07 +
                                                                z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))))));
    const int n = (k == k && fabs(k) < 1e18) ? (int)((long long)k & 3) : 0;
    sn = n == 0 ? s : n == 1 ? c : n == 2 ? -s : -c;
    cs = n == 0 ? c : n == 1 ? -s : n == 2 ? -c : s;
}

__device__ __forceinline__ double atan_pos(double ax) {
    const int idx = ax < 0.4375 ? -1 : ax < 0.6875 ? 0 : ax < 1.1875 ? 1 : ax < 2.4375 ? 2 : 3;
    const double t = idx == -1 ? ax
                     : idx == 0 ? (2.0 * ax - 1.0) / (2.0 + ax)
                     : idx == 1 ? (ax - 1.0) / (ax + 1.0)
                     : idx == 2 ? (ax - 1.5) / (1.0 + 1.5 * ax)
                                : -1.0 / ax;
    const double z = t * t, w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 +
                           w * (1.42857142725034663711e-01 +
                                w * (9.09088713343650656196e-02 + w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 +
                           w * (-1.11111104054623557880e-01 +
                                w * (-7.69187620504482999495e-02 + w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    if (idx == -1) return t - t * (s1 + s2);
    const double hi = idx == 0 ? 4.63647609000806093515e-01 : idx == 1 ? 7.85398163397448278999e-01 : idx == 2 ? 9.82793723247329054082e-01 : 1.57079632679489655800e+00;
    const double lo = idx == 0 ? 2.26987774529616870924e-17 : idx == 1 ? 3.06161699786838301793e-17 : idx == 2 ? 1.39033110312309984516e-17 : 6.12323399573676603587e-17;
    return hi - ((t * (s1 + s2) - lo) - t);
}

__device__ __forceinline__ double atan2_d(double y, double x) {
    const double pi = 3.1415926535897931160e+00, piLo = 1.2246467991473531772e-16;
    const double a = atan_pos(fabs(y / x));
    const double r = x == 0 ? (y == 0 ? 0.0 : 0.5 * pi) : x > 0 ? a : pi - (a - piLo);
    return y < 0 ? -r : r;
}

// ---- SE3Quat (Thirdparty/g2o/g2o/types/se3quat.h) with Eigen's quaternion ---------------------------------------------------------
__device__ __forceinline__ void normalize_q(double q[4]) {  // normalizeRotation()
    if (q[3] < 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) q[i] = q[i] * -1.0;
    }
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = q[i] / n;
}

// Quaternion * vector: uv = 2 vec x v; v + w uv + vec x uv
__device__ __forceinline__ void rot(const double q[4], const double v[3], double o[3]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    double ux = y * v[2] - z * v[1], uy = z * v[0] - x * v[2], uz = x * v[1] - y * v[0];
    ux = ux + ux, uy = uy + uy, uz = uz + uz;
    o[0] = (v[0] + w * ux) + (y * uz - z * uy);
    o[1] = (v[1] + w * uy) + (z * ux - x * uz);
    o[2] = (v[2] + w * uz) + (x * uy - y * ux);
}

__device__ __forceinline__ void map(const Se3d &T, const double v[3], double o[3]) {  // _r * xyz + _t
    rot(T.q, v, o);
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = o[i] + T.t[i];
}

__device__ __forceinline__ Se3d mul(const Se3d &A, const Se3d &B) {  // operator*: t = tA + rA * tB, r = rA * rB, normalised
    Se3d R;
    const double ax = A.q[0], ay = A.q[1], az = A.q[2], aw = A.q[3], bx = B.q[0], by = B.q[1], bz = B.q[2], bw = B.q[3];
    R.q[0] = aw * bx + ax * bw + ay * bz - az * by;
    R.q[1] = aw * by + ay * bw + az * bx - ax * bz;
    R.q[2] = aw * bz + az * bw + ax * by - ay * bx;
    R.q[3] = aw * bw - ax * bx - ay * by - az * bz;
    normalize_q(R.q);
    double r[3];
    rot(A.q, B.t, r);
#pragma unroll
    for (int i = 0; i < 3; i++) R.t[i] = A.t[i] + r[i];
    return R;
}

__device__ __forceinline__ void to_rot(const double q[4], double R[9]) {  // toRotationMatrix()
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
    R[3] = txy + twz, R[4] = 1.0 - (txx + tzz), R[5] = tyz - twx;
    R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0 - (txx + tyy);
}

__device__ __forceinline__ void quat_of(const double R[9], double q[4]) {  // Quaterniond(Matrix3d)
    double t = (R[0] + R[4]) + R[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t, q[1] = (R[2] - R[6]) * t, q[2] = (R[3] - R[1]) * t;
        return;
    }
    // i: the largest diagonal entry; (i, j, k) cyclic.  Written out per i: no indexed registers
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > (i == 1 ? R[4] : R[0])) i = 2;
    if (i == 0) {
        t = sqrt(R[0] - R[4] - R[8] + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[7] - R[5]) * t, q[1] = (R[3] + R[1]) * t, q[2] = (R[6] + R[2]) * t;
    } else if (i == 1) {
        t = sqrt(R[4] - R[8] - R[0] + 1.0);
        q[1] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[2] - R[6]) * t, q[2] = (R[7] + R[5]) * t, q[0] = (R[1] + R[3]) * t;
    } else {
        t = sqrt(R[8] - R[0] - R[4] + 1.0);
        q[2] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[3] - R[1]) * t, q[0] = (R[2] + R[6]) * t, q[1] = (R[5] + R[7]) * t;
    }
}

// SE3Quat::exp (se3quat.h:223-257): omega = u[0..2], upsilon = u[3..5]
__device__ __forceinline__ Se3d se3_exp(const double u[6]) {
    const double ox = u[0], oy = u[1], oz = u[2];
    const double theta = sqrt((ox * ox + oy * oy) + oz * oz);
    const double Om[9] = {0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0};
    double Om2[9], R[9], V[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Om2[3 * i + j] = (Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j];
    if (theta < 0.00001) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + Om[i]) + Om2[i], V[i] = R[i];
    } else {
        double sn, cs;
        sincos_d(theta, sn, cs);
        const double a = sn / theta, b = (1.0 - cs) / (theta * theta), c = (theta - sn) / (theta * theta * theta);
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const double I = i % 4 == 0 ? 1.0 : 0.0;
            R[i] = (I + a * Om[i]) + b * Om2[i];
            V[i] = (I + b * Om[i]) + c * Om2[i];
        }
    }
    Se3d E;
#pragma unroll
    for (int i = 0; i < 3; i++) E.t[i] = (V[3 * i] * u[3] + V[3 * i + 1] * u[4]) + V[3 * i + 2] * u[5];
    quat_of(R, E.q);
    normalize_q(E.q);
    return E;
}

// ---- cameras: parameters are floats promoted to double ---------------------------------------------------------------------------
// pCamera->project(Vector3d): Pinhole.cpp:35; KannalaBrandt8.cpp:46-63 - theta and psi through float atan2f / sqrtf, then double cos / sin
__device__ __forceinline__ void project(int model, const float *cam, const double P[3], double uv[2]) {
    if (model == 0) {
        uv[0] = (double)cam[0] * P[0] / P[2] + (double)cam[2];
        uv[1] = (double)cam[1] * P[1] / P[2] + (double)cam[3];
        return;
    }
    const double r2 = P[0] * P[0] + P[1] * P[1];
    const double theta = (double)ft_libm::atan2f_glibc(sqrtf((float)r2), (float)P[2]);
    const double psi = (double)ft_libm::atan2f_glibc((float)P[1], (float)P[0]);
    const double t2 = theta * theta, t3 = theta * t2, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
    const double r = theta + (double)cam[4] * t3 + (double)cam[5] * t5 + (double)cam[6] * t7 + (double)cam[7] * t9;
    double sn, cs;
    sincos_d(psi, sn, cs);
    uv[0] = (double)cam[0] * r * cs + (double)cam[2];
    uv[1] = (double)cam[1] * r * sn + (double)cam[3];
}

// pCamera->projectJac(Vector3d): Pinhole.cpp:71-81, KannalaBrandt8.cpp:145-175 (3 * k0 ... 9 * k3 are float products)
__device__ __forceinline__ void project_jac(int model, const float *cam, const double P[3], double J[6]) {
    const double x = P[0], y = P[1], z = P[2];
    if (model == 0) {
        J[0] = (double)cam[0] / z, J[1] = 0.0, J[2] = -(double)cam[0] * x / (z * z);
        J[3] = 0.0, J[4] = (double)cam[1] / z, J[5] = -(double)cam[1] * y / (z * z);
        return;
    }
    const double x2 = x * x, y2 = y * y, z2 = z * z;
    const double r2 = x2 + y2, r = sqrt(r2), r3 = r2 * r;
    const double th = atan2_d(r, z);
    const double th2 = th * th, th3 = th2 * th, th4 = th2 * th2, th5 = th4 * th, th6 = th2 * th4, th7 = th6 * th, th8 = th4 * th4, th9 = th8 * th;
    const double f = th + th3 * (double)cam[4] + th5 * (double)cam[5] + th7 * (double)cam[6] + th9 * (double)cam[7];
    const double k3 = (double)__fmul_rn(3.f, cam[4]), k5 = (double)__fmul_rn(5.f, cam[5]), k7 = (double)__fmul_rn(7.f, cam[6]), k9 = (double)__fmul_rn(9.f, cam[7]);
    const double fd = 1 + k3 * th2 + k5 * th4 + k7 * th6 + k9 * th8;
    const double den = r2 * (r2 + z2);
    const double fx = (double)cam[0], fy = (double)cam[1];
    J[0] = fx * (fd * z * x2 / den + f * y2 / r3);
    J[3] = fy * (fd * z * y * x / den - f * y * x / r3);
    J[1] = fx * (fd * z * y * x / den - f * y * x / r3);
    J[4] = fy * (fd * z * y2 / den + f * x2 / r3);
    J[2] = -fx * fd * x / (r2 + z2);
    J[5] = -fy * fd * y / (r2 + z2);
}

// what a thread needs of its frame besides the estimate
struct FrameConst {
    const FtPoseOptJob *job;
    Se3d Trl;
    double Rrl[9];
    double bf;
};

// computeError of edge E at the estimate (estR = mTrl * estimate, read by the to-body edge) -> e[3] (e[2] = 0 for the mono edges)
__device__ __forceinline__ void edge_error(const FrameConst &F, const FtPoseEdge &E, const Se3d &est, const Se3d &estR, double e[3]) {
    const FtPoseOptJob *J = F.job;
    const double X[3] = {(double)E.X[0], (double)E.X[1], (double)E.X[2]};
    double P[3], uv[2];
    if (E.kind == 2) {
        map(est, X, P);
        const double invz = (double)(float)(1.0 / P[2]);  // const float invz = 1.0f / trans_xyz[2]
        const double u = P[0] * invz * (double)J->cam[0] + (double)J->cam[2];
        const double v = P[1] * invz * (double)J->cam[1] + (double)J->cam[3];
        e[0] = (double)E.obs[0] - u;
        e[1] = (double)E.obs[1] - v;
        e[2] = (double)E.obs[2] - (u - F.bf * invz);
        return;
    }
    if (E.kind == 0) {
        map(est, X, P);
        project(J->model, J->cam, P, uv);
    } else {
        map(estR, X, P);
        project(J->model, J->cam2, P, uv);
    }
    e[0] = (double)E.obs[0] - uv[0];
    e[1] = (double)E.obs[1] - uv[1];
    e[2] = 0.0;
}

// _error.dot(information() * _error)
__device__ __forceinline__ double edge_chi2(const double e[3], double w, bool dim3) {
    const double c = e[0] * (w * e[0]) + e[1] * (w * e[1]);
    return dim3 ? c + e[2] * (w * e[2]) : c;
}

// RobustKernelHuber::robustify: delta a float, dsqr a float (robust_kernel_impl.h:84) -> rho[0], rho[1]
__device__ __forceinline__ void huber(double chi2, bool stereo, double &rho0, double &rho1) {
    const float deltaF = stereo ? (float)sqrt(7.815) : (float)sqrt(5.991);
    const double delta = (double)deltaF, dsqr = (double)(float)(delta * delta);
    if (chi2 <= dsqr) {
        rho0 = chi2, rho1 = 1.0;
    } else {
        const double sq = sqrt(chi2);
        rho0 = 2 * sq * delta - dsqr;
        rho1 = delta / sq;
    }
}

// linearizeOplus of edge E -> A[3][6] (row 2 zero for the mono edges)
__device__ __forceinline__ void edge_jacobian(const FrameConst &F, const FtPoseEdge &E, const Se3d &est, double A[18]) {
    const FtPoseOptJob *J = F.job;
    const double X[3] = {(double)E.X[0], (double)E.X[1], (double)E.X[2]};
    double P[3];
    map(est, X, P);
    const double x = P[0], y = P[1], z = P[2];
    if (E.kind == 2) {
        const double fx = (double)J->cam[0], fy = (double)J->cam[1], bf = F.bf;
        const double invz = 1.0 / z, invz_2 = invz * invz;
        A[0] = x * y * invz_2 * fx;
        A[1] = -(1 + (x * x * invz_2)) * fx;
        A[2] = y * invz * fx;
        A[3] = -invz * fx;
        A[4] = 0;
        A[5] = x * invz_2 * fx;
        A[6] = (1 + y * y * invz_2) * fy;
        A[7] = -x * y * invz_2 * fy;
        A[8] = -x * invz * fy;
        A[9] = 0;
        A[10] = -invz * fy;
        A[11] = y * invz_2 * fy;
        A[12] = A[0] - bf * y * invz_2;
        A[13] = A[1] + bf * x * invz_2;
        A[14] = A[2];
        A[15] = A[3];
        A[16] = 0;
        A[17] = A[5] - bf * invz_2;
        return;
    }
    const double S[18] = {0.0, z, -y, 1.0, 0.0, 0.0, -z, 0.0, x, 0.0, 1.0, 0.0, y, -x, 0.0, 0.0, 0.0, 1.0};  // SE3deriv
    double Jc[6], L[6];
    if (E.kind == 0) {
        project_jac(J->model, J->cam, P, Jc);
#pragma unroll
        for (int i = 0; i < 6; i++) L[i] = -Jc[i];
    } else {
        double Pr[3];
        map(F.Trl, P, Pr);  // mTrl.map(T_lw.map(Xw))
        project_jac(J->model, J->cam2, Pr, Jc);
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) L[3 * r + c] = (-Jc[3 * r] * F.Rrl[c] + -Jc[3 * r + 1] * F.Rrl[3 + c]) + -Jc[3 * r + 2] * F.Rrl[6 + c];
    }
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 6; c++) A[6 * r + c] = (L[3 * r] * S[c] + L[3 * r + 1] * S[6 + c]) + L[3 * r + 2] * S[12 + c];
#pragma unroll
    for (int c = 0; c < 6; c++) A[12 + c] = 0.0;
}

// 6 x 6 LDLT of the lower triangle H (row by row: 21) with lambda on the diagonal, no pivoting; a factor that is not > 0 fails
// (linear_solver_dense.h:104-112: isPositive()).  x is written only on success.
__device__ __forceinline__ bool ldlt_solve(const double Hs[21], double lambda, const double b[6], double x[6]) {
    double H[6][6], L[6][6], d[6], y[6], zz[6];
#pragma unroll
    for (int i = 0, c = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++, c++) H[i][j] = i == j ? Hs[c] + lambda : Hs[c];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double s = H[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) s = s - L[j][k] * (L[j][k] * d[k]);
        d[j] = s;
        if (!(s > 0)) ok = false;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = H[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) v = v - L[i][k] * (L[j][k] * d[k]);
            L[i][j] = v / d[j];
        }
    }
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
        y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) zz[i] = y[i] / d[i];
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = zz[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s = s - L[k][i] * x[k];
        x[i] = s;
    }
    return true;
}

// One evaluation of the active edges at `est`: computeActiveErrors + activeRobustChi2, and with FULL also buildSystem.  Every
// thread returns the same sums: tot[0] chi2, tot[1..21] H, tot[22..27] -b.  An edge that is not active adds exact zeros.
template <bool FULL>
__device__ __forceinline__ void evaluate(const FrameConst &F, const FtPoseEdge *edges, float *chi2f, const uint8_t *level, int nE, const Se3d &est,
                                         bool twoCam, bool robust, double *buf, double *totLds, double tot[FT_POSE_TERMS]) {
    const int tid = threadIdx.x;
    constexpr int NT = FULL ? FT_POSE_TERMS : 1;
    Se3d estR = est;
    if (twoCam) estR = mul(F.Trl, est);  // (mTrl * v1->estimate())
    double acc = 0.0;
    for (int base = 0; base < nE; base += FT_POSE_T) {
        const int e = base + tid;
        double term[NT];
#pragma unroll
        for (int k = 0; k < NT; k++) term[k] = 0.0;
        if (e < nE && level[e] == 0) {
            const FtPoseEdge E = edges[e];
            const bool stereo = E.kind == 2;
            const double w = (double)E.w;
            double er[3];
            edge_error(F, E, est, estR, er);
            const double chi2 = edge_chi2(er, w, stereo);
            chi2f[e] = (float)chi2;  // const float chi2 = e->chi2() of the classification, should this be the last evaluation
            double rho0 = chi2, rho1 = 1.0;
            if (robust) huber(chi2, stereo, rho0, rho1);
            term[0] = rho0;
            if (FULL) {
                double A[18];
                edge_jacobian(F, E, est, A);
                const double wr = rho1 * w;
                int c = 1;
#pragma unroll
                for (int i = 0; i < 6; i++)
#pragma unroll
                    for (int j = 0; j <= i; j++, c++) {
                        const double s = (A[i] * wr) * A[j] + (A[6 + i] * wr) * A[6 + j];
                        term[c] = stereo ? s + (A[12 + i] * wr) * A[12 + j] : s;
                    }
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    const double s = ((rho1 * A[j]) * w) * er[0] + ((rho1 * A[6 + j]) * w) * er[1];
                    term[22 + j] = stereo ? s + ((rho1 * A[12 + j]) * w) * er[2] : s;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NT; k++) buf[tid * FT_POSE_PITCH + k] = term[k];
        __syncthreads();
        if (tid < NT) {
            const int n = min(FT_POSE_T, nE - base);
#pragma unroll 8
            for (int i = 0; i < n; i++) acc = acc + buf[i * FT_POSE_PITCH + tid];
        }
        __syncthreads();
    }
    if (tid < NT) totLds[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NT; k++) tot[k] = totLds[k];
    __syncthreads();
}

__global__ __launch_bounds__(FT_POSE_T) void k_pose_opt(FtPoseOptCall T) {
    __shared__ double buf[FT_POSE_T * FT_POSE_PITCH];
    __shared__ double totLds[FT_POSE_TERMS];
    __shared__ int nBadLds;
    const int tid = threadIdx.x;
    const FtPoseOptJob *job = (const FtPoseOptJob *)(T.arena + T.jobs) + blockIdx.x;
    const int nE = job->nE;
    const FtPoseEdge *edges = (const FtPoseEdge *)(T.arena + job->edges);
    float *chi2f = (float *)(T.arena + job->work);
    uint8_t *level = (uint8_t *)(chi2f + nE);
    uint8_t *flags = T.arena + job->flags;
    FtPoseOptOut *out = (FtPoseOptOut *)(T.arena + job->out);

    FrameConst F;
    F.job = job;
    F.bf = (double)job->bf;
    bool twoCam = false;
    for (int e = tid; e < nE; e += FT_POSE_T) level[e] = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) F.Trl.q[i] = (double)job->trlQ[i];
#pragma unroll
    for (int i = 0; i < 3; i++) F.Trl.t[i] = (double)job->trlT[i];
    normalize_q(F.Trl.q);
    to_rot(F.Trl.q, F.Rrl);
    twoCam = job->twoCam != 0;
    Se3d est0;
#pragma unroll
    for (int i = 0; i < 4; i++) est0.q[i] = (double)job->q[i];
#pragma unroll
    for (int i = 0; i < 3; i++) est0.t[i] = (double)job->t[i];
    normalize_q(est0.q);

    Se3d est = est0;
    bool robust = true;
    int nBad = 0;
    int itsOut[4] = {0, 0, 0, 0}, rejOut[4] = {0, 0, 0, 0};
    double chiOut[4] = {0.0, 0.0, 0.0, 0.0};
    for (int rnd = 0; rnd < 4; rnd++) {
        est = est0;  // :1008-1009: every round starts from the frame's pose
        int its = 0, rej = 0;
        double cur = 0.0;
        if (nE - nBad > 0) {  // initializeOptimization(0): the edges of level 0
            double lambda = 0.0, ni = 0.0;
            int lmBad = 0;
            double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int it = 0; it < 10; it++) {
                double tot[FT_POSE_TERMS];
                evaluate<true>(F, edges, chi2f, level, nE, est, twoCam, robust, buf, totLds, tot);
                cur = tot[0];
                const double ini = cur;
                double b[6];
#pragma unroll
                for (int j = 0; j < 6; j++) b[j] = -tot[22 + j];
                if (it == 0) {  // computeLambdaInit: _tau * max |H_jj|
                    double m = 0.0;
#pragma unroll
                    for (int j = 0, c = 0; j < 6; c += j + 2, j++) m = fmax(fabs(tot[1 + c]), m);
                    lambda = 1e-5 * m;
                    ni = 2.0;
                    lmBad = 0;
                }
                double rho = 0.0;
                int qmax = 0;
                const Se3d backup = est;
                do {
                    const bool ok2 = ldlt_solve(tot + 1, lambda, b, x);
                    est = mul(se3_exp(x), est);  // oplusImpl: SE3Quat::exp(update) * estimate()
                    double t1[1];
                    evaluate<false>(F, edges, chi2f, level, nE, est, twoCam, robust, buf, totLds, t1);
                    double tmp = t1[0];
                    if (!ok2) tmp = 1.7976931348623157e308;
                    rho = cur - tmp;
                    double scale = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
                    scale += 1e-3;
                    rho /= scale;
                    if (rho > 0 && isfinite(tmp)) {
                        const double t = 2 * rho - 1;
                        const double alpha = fmin(1.0 - t * t * t, 2.0 / 3.0);
                        lambda *= fmax(1.0 / 3.0, alpha);
                        ni = 2.0;
                        cur = tmp;
                    } else {
                        lambda *= ni;
                        ni *= 2;
                        est = backup;  // pop(): the vertex, not the errors
                        rej++;
                    }
                    qmax++;
                } while (rho < 0 && qmax < 10);
                its++;
                if (qmax == 10 || rho == 0) break;
                if ((ini - cur) * 1e3 < ini) lmBad++;
                else lmBad = 0;
                if (lmBad >= 3) break;
            }
        }
        itsOut[rnd] = its, rejOut[rnd] = rej, chiOut[rnd] = cur;
        // :1014-1100: an outlier's error is recomputed at the final estimate, an inlier's chi2 is what the last evaluation left
        if (tid == 0) nBadLds = 0;
        __syncthreads();
        {
            Se3d estR = est;
            if (twoCam) estR = mul(F.Trl, est);
            int bad = 0;
            for (int e = tid; e < nE; e += FT_POSE_T) {
                const FtPoseEdge E = edges[e];
                const bool stereo = E.kind == 2;
                float c = chi2f[e];
                if (level[e]) {
                    double er[3];
                    edge_error(F, E, est, estR, er);
                    c = (float)edge_chi2(er, (double)E.w, stereo);
                }
                const uint8_t o = c > (stereo ? 7.815f : 5.991f) ? 1 : 0;
                level[e] = o;
                flags[e] = o;
                bad += o;
            }
            if (bad) atomicAdd(&nBadLds, bad);
        }
        __syncthreads();
        nBad = nBadLds;
        __syncthreads();
        if (rnd == 2) robust = false;
        if (nE < 10) break;  // optimizer.edges().size() < 10
    }
    if (tid == 0) {
        // Sophus::SE3<float>(rotation().cast<float>(), translation().cast<float>()): the float quaternion is normalised
        const float q[4] = {(float)est.q[0], (float)est.q[1], (float)est.q[2], (float)est.q[3]};
        const float n = sqrtf(__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(q[0], q[0]), __fmul_rn(q[1], q[1])), __fmul_rn(q[2], q[2])), __fmul_rn(q[3], q[3])));
        for (int i = 0; i < 4; i++) out->q[i] = __fdiv_rn(q[i], n);
        for (int i = 0; i < 3; i++) out->t[i] = (float)est.t[i];
        out->ret = nE - nBad;
        for (int i = 0; i < 4; i++) out->iterations[i] = itsOut[i], out->rejected[i] = rejOut[i], out->chi[i] = chiOut[i];
    }
}

}  // namespace

int ft_launch_pose_opt(hipStream_t st, const FtPoseOptCall &T) {
    hipLaunchKernelGGL(k_pose_opt, dim3((unsigned)T.nJobs), dim3(FT_POSE_T), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

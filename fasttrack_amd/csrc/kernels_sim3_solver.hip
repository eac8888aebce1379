// HIP kernels of Sim3Solver (reference src/Sim3Solver.cc) for gfx950 (wave64): the RANSAC of Horn's closed-form Sim3 that loop
// closing runs per candidate (src/LoopClosing.cc:698-710) - every hypothesis of every problem of a call in three launches.
//   k_sim3_hypotheses  blockIdx.y = job, a LANE per iteration.  The three draws of the iteration become three pair indices
//                      (DUtils::Random::RandomInt and the swap-with-back removal of :177-185 on a fresh index list, in closed form),
//                      then ComputeSim3 (:311-414): all float steps in the reference's order, the eigenvector of the 4 x 4 N by a
//                      cyclic two-sided Jacobi in double (largest_eigenvector4: NOT Eigen's EigenSolver, see fasttrack_amd.h),
//                      atan2f / sinf / cosf as glibc evaluates them (libm_f32.h), Sophus::SO3f::exp with its small-angle branch.
//                      It leaves mT12i, mT21i, mR12i, ms12i of the iteration in the job's FtSim3Hyp array.
//   k_sim3_count       blockIdx.y = job, a WAVE per iteration (four per workgroup).  CheckInliers (:417-441): the lanes stride over
//                      the pair records, mnInliersi is the sum of the ballots' population counts.  The pairs are independent and
//                      the count is an integer: no order of the lanes changes it.
//   k_sim3_select      blockIdx.x = job.  The sequential selection of iterate (:240-293) evaluated on the counts: the run stops at
//                      the first iteration whose count exceeds min_inliers (else at the last); the best is the LAST iteration up to
//                      the stop that holds the largest count of that prefix (the test at :265 is >=).  The winner is evaluated once
//                      more for mvbBestInliers; its transform goes to the job's result.
// Contraction is off (Makefile) and every float step is an __f*_rn intrinsic, so each expression is evaluated as written;
// tests/sim3_solver_ref.py is the same text in numpy.  A NaN or infinite scale (a sample of coincident points: den == 0) makes
// every error NaN, `err < max` false and the count 0, as IEEE arithmetic makes the reference behave: no test below asks isnan.
#include "ft_internal.h"
#include "ft_search.h"
#include "kb8_triangulate.h"

namespace {

#define FT_S3_WAVES 4  // iterations per workgroup of k_sim3_count

__device__ __forceinline__ float sum3(float e0, float e1, float e2) { return __fadd_rn(e0, __fadd_rn(e1, e2)); }  // Eigen: e0 + (e1 + e2)

// Eigenvector of the largest eigenvalue of the symmetric 4 x 4 A (row-major), the first on a tie, with q[0] >= 0, narrowed to
// float.  Cyclic two-sided Jacobi in double: sweeps over the pivots (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a pivot is rotated away
// unless it is 0 or not above 1e-18 (|app| + |aqq|); the sweeps end with the first that rotates nothing, or after 30.
__device__ void largest_eigenvector4(const double N[16], float q[4]) {
    double A[16], V[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        A[i] = N[i];
        V[i] = (i % 5 == 0) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int r = p + 1; r < 4; r++) {
                const double apq = A[4 * p + r], app = A[5 * p], aqq = A[5 * r];
                if (apq == 0.0 || !(fabs(apq) > __dmul_rn(1e-18, __dadd_rn(fabs(app), fabs(aqq))))) continue;
                rotated = true;
                const double theta = __ddiv_rn(__dsub_rn(aqq, app), __dmul_rn(2.0, apq));
                const double t = __ddiv_rn(theta >= 0 ? 1.0 : -1.0, __dadd_rn(fabs(theta), sqrt(__dadd_rn(__dmul_rn(theta, theta), 1.0))));
                const double c = __ddiv_rn(1.0, sqrt(__dadd_rn(__dmul_rn(t, t), 1.0))), s = __dmul_rn(t, c);
                A[5 * p] = __dsub_rn(app, __dmul_rn(t, apq));
                A[5 * r] = __dadd_rn(aqq, __dmul_rn(t, apq));
                A[4 * p + r] = A[4 * r + p] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (k != p && k != r) {
                        const double akp = A[4 * k + p], akq = A[4 * k + r];
                        A[4 * k + p] = A[4 * p + k] = __dsub_rn(__dmul_rn(c, akp), __dmul_rn(s, akq));
                        A[4 * k + r] = A[4 * r + k] = __dadd_rn(__dmul_rn(s, akp), __dmul_rn(c, akq));
                    }
                    const double vkp = V[4 * k + p], vkq = V[4 * k + r];
                    V[4 * k + p] = __dsub_rn(__dmul_rn(c, vkp), __dmul_rn(s, vkq));
                    V[4 * k + r] = __dadd_rn(__dmul_rn(s, vkp), __dmul_rn(c, vkq));
                }
            }
        if (!rotated) break;
    }
    int best = 0;
    double top = A[0];
#pragma unroll
    for (int j = 1; j < 4; j++)
        if (A[5 * j] > top) top = A[5 * j], best = j;
    double v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = best == 0 ? V[4 * i] : best == 1 ? V[4 * i + 1] : best == 2 ? V[4 * i + 2] : V[4 * i + 3];
    const bool flip = v[0] < 0;
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = (float)(flip ? -v[i] : v[i]);
}

// DUtils::Random::RandomInt(0, d - 1) of the draw r: int(((double)r / ((double)RAND_MAX + 1.0)) * d)
__device__ __forceinline__ int random_int(int r, int d) { return (int)__dmul_rn(__ddiv_rn((double)r, 2147483648.0), (double)d); }

// ComputeCentroid (:302-308): C = P.rowwise().sum() / 3; Pr.col(i) = P.col(i) - C.  P[i] is column i.
__device__ __forceinline__ void centroid(const float P[3][3], float Pr[3][3], float C[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) C[k] = __fdiv_rn(sum3(P[0][k], P[1][k], P[2][k]), 3.f);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) Pr[i][k] = __fsub_rn(P[i][k], C[k]);
}

// Quaternionf(w, x, y, z).toRotationMatrix() (Eigen/src/Geometry/Quaternion.h), row-major
__device__ __forceinline__ void quat_matrix(float w, float x, float y, float z, float R[9]) {
    const float tx = __fmul_rn(2.f, x), ty = __fmul_rn(2.f, y), tz = __fmul_rn(2.f, z);
    const float twx = __fmul_rn(tx, w), twy = __fmul_rn(ty, w), twz = __fmul_rn(tz, w);
    const float txx = __fmul_rn(tx, x), txy = __fmul_rn(ty, x), txz = __fmul_rn(tz, x);
    const float tyy = __fmul_rn(ty, y), tyz = __fmul_rn(tz, y), tzz = __fmul_rn(tz, z);
    R[0] = __fsub_rn(1.f, __fadd_rn(tyy, tzz)), R[1] = __fsub_rn(txy, twz), R[2] = __fadd_rn(txz, twy);
    R[3] = __fadd_rn(txy, twz), R[4] = __fsub_rn(1.f, __fadd_rn(txx, tzz)), R[5] = __fsub_rn(tyz, twx);
    R[6] = __fsub_rn(txz, twy), R[7] = __fadd_rn(tyz, twx), R[8] = __fsub_rn(1.f, __fadd_rn(txx, tyy));
}

// ComputeSim3 (:311-414).  P1[i], P2[i]: the sample's points (columns of P3Dc1i, P3Dc2i)
__device__ void compute_sim3(const float P1[3][3], const float P2[3][3], bool fixScale, FtSim3Hyp &H) {
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
    centroid(P1, Pr1, O1);
    centroid(P2, Pr2, O2);
    float M[3][3];  // M = Pr2 * Pr1.transpose(): M(i, j) = sum over the points k of Pr2(i, k) Pr1(j, k)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            M[i][j] = sum3(__fmul_rn(Pr2[0][i], Pr1[0][j]), __fmul_rn(Pr2[1][i], Pr1[1][j]), __fmul_rn(Pr2[2][i], Pr1[2][j]));
    // :335-349: float sums, held in doubles, narrowed into the Matrix4f
    const float N11 = __fadd_rn(__fadd_rn(M[0][0], M[1][1]), M[2][2]), N12 = __fsub_rn(M[1][2], M[2][1]), N13 = __fsub_rn(M[2][0], M[0][2]),
                N14 = __fsub_rn(M[0][1], M[1][0]), N22 = __fsub_rn(__fsub_rn(M[0][0], M[1][1]), M[2][2]), N23 = __fadd_rn(M[0][1], M[1][0]),
                N24 = __fadd_rn(M[2][0], M[0][2]), N33 = __fsub_rn(__fadd_rn(-M[0][0], M[1][1]), M[2][2]), N34 = __fadd_rn(M[1][2], M[2][1]),
                N44 = __fadd_rn(__fsub_rn(-M[0][0], M[1][1]), M[2][2]);
    const double Nd[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    float q[4];
    largest_eigenvector4(Nd, q);
    float vec[3] = {q[1], q[2], q[3]};
    const float nv = fnorm3(vec);
    const float ang = ft_atan2_f(nv, q[0]);
    if (nv != 0) {  // vec = 2 * ang * vec / vec.norm()
        const float k = __fmul_rn(2.f, ang);
#pragma unroll
        for (int i = 0; i < 3; i++) vec[i] = __fdiv_rn(__fmul_rn(k, vec[i]), nv);
    }
    // Sophus::SO3f::expAndTheta (so3.hpp:583-619), Constants<float>::epsilon() = 1e-5f
    const float thetaSq = fdot3(vec, vec);
    float imag, real;
    if (thetaSq < __fmul_rn(1e-5f, 1e-5f)) {
        const float po4 = __fmul_rn(thetaSq, thetaSq);
        imag = __fadd_rn(__fsub_rn(0.5f, __fmul_rn((float)(1.0 / 48.0), thetaSq)), __fmul_rn((float)(1.0 / 3840.0), po4));
        real = __fadd_rn(__fsub_rn(1.f, __fmul_rn((float)(1.0 / 8.0), thetaSq)), __fmul_rn((float)(1.0 / 384.0), po4));
    } else {
        const float theta = sqrtf(thetaSq), half = __fmul_rn(0.5f, theta);
        imag = __fdiv_rn(ft_sin_f(half), theta);
        real = ft_cos_f(half);
    }
    float *R = H.R;
    quat_matrix(real, __fmul_rn(imag, vec[0]), __fmul_rn(imag, vec[1]), __fmul_rn(imag, vec[2]), R);
    float P3[3][3];  // P3 = R * Pr2, column i
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) P3[i][k] = fdot3(R + 3 * k, Pr2[i]);
    float s = 1.0f;
    if (!fixScale) {  // the nine terms in column-major order, one after the other
        float nom = 0.f, den = 0.f;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float a = __fmul_rn(Pr1[i][k], P3[i][k]), b = __fmul_rn(P3[i][k], P3[i][k]);
                nom = (i == 0 && k == 0) ? a : __fadd_rn(nom, a);
                den = (i == 0 && k == 0) ? b : __fadd_rn(den, b);
            }
        s = (float)__ddiv_rn((double)nom, (double)den);
    }
    H.s = s;
    float sR[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; i++) sR[i] = __fmul_rn(s, R[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = __fsub_rn(O1[i], fdot3(sR + 3 * i, O2));  // mt12i = O1 - ms12i * mR12i * O2
    const float inv = (float)__ddiv_rn(1.0, (double)s);
    float nsRinv[9];  // -sRinv, sRinv = (1.0 / ms12i) * mR12i.transpose()
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float v = __fmul_rn(inv, R[3 * j + i]);
            H.T21[4 * i + j] = v;
            nsRinv[3 * i + j] = -v;
            H.T12[4 * i + j] = sR[3 * i + j];
        }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        H.T12[4 * i + 3] = t[i];
        H.T21[4 * i + 3] = fdot3(nsRinv + 3 * i, t);  // tinv = -sRinv * mt12i
    }
    H.pad[0] = H.pad[1] = 0.f;
}

// pCamera->project(Eigen::Vector3f) (Pinhole.cpp:43-49, KannalaBrandt8.cpp:67-84); neither tests the depth
__device__ __forceinline__ void project(int model, const float *cam, const float p[3], float uv[2]) {
    if (model == 0) {
        uv[0] = __fadd_rn(__fdiv_rn(__fmul_rn(cam[0], p[0]), p[2]), cam[2]);
        uv[1] = __fadd_rn(__fdiv_rn(__fmul_rn(cam[1], p[1]), p[2]), cam[3]);
    } else {
        kb8_project(cam, p, uv);
    }
}

// one pair of CheckInliers (:417-441) under the hypothesis (T12, T21)
__device__ __forceinline__ bool pair_is_inlier(const FtSim3SolverJob *J, const float *T12, const float *T21, const FtSim3Pair &P) {
    float a[3], b[3], u1[2], u2[2];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        a[i] = __fadd_rn(fdot3(T12 + 4 * i, P.X2), T12[4 * i + 3]);  // Project(mvX3Dc2, vP2im1, mT12i, pCamera1)
        b[i] = __fadd_rn(fdot3(T21 + 4 * i, P.X1), T21[4 * i + 3]);  // Project(mvX3Dc1, vP1im2, mT21i, pCamera2)
    }
    project(J->model1, J->cam1, a, u1);
    project(J->model2, J->cam2, b, u2);
    const float d1x = __fsub_rn(P.P1[0], u1[0]), d1y = __fsub_rn(P.P1[1], u1[1]);
    const float d2x = __fsub_rn(u2[0], P.P2[0]), d2y = __fsub_rn(u2[1], P.P2[1]);
    const float err1 = __fadd_rn(__fmul_rn(d1x, d1x), __fmul_rn(d1y, d1y));
    const float err2 = __fadd_rn(__fmul_rn(d2x, d2x), __fmul_rn(d2y, d2y));
    return err1 < P.max1 && err2 < P.max2;
}

__global__ __launch_bounds__(64) void k_sim3_hypotheses(FtSim3SolverCall T) {
    const FtSim3SolverJob *J = (const FtSim3SolverJob *)(T.arena + T.jobs) + blockIdx.y;
    const int it = blockIdx.x * 64 + threadIdx.x;
    if (it >= J->eff) return;
    const FtSim3Pair *pairs = (const FtSim3Pair *)(T.arena + J->pairs);
    const int *draws = (const int *)(T.arena + J->draws) + 3 * it;
    const int N = J->N;  // >= 3
    // :172-186 on vAvailableIndices = 0 .. N - 1: position r0 then holds N - 1; the back of the second list is position N - 2
    const int r0 = random_int(draws[0], N), r1 = random_int(draws[1], N - 1), r2 = random_int(draws[2], N - 2);
    const int back1 = (N - 2 == r0) ? N - 1 : N - 2;
    const int idx[3] = {r0, r1 == r0 ? N - 1 : r1, r2 == r1 ? back1 : r2 == r0 ? N - 1 : r2};
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) P1[i][k] = pairs[idx[i]].X1[k], P2[i][k] = pairs[idx[i]].X2[k];
    FtSim3Hyp H;
    compute_sim3(P1, P2, J->fixScale != 0, H);
    ((FtSim3Hyp *)(T.arena + J->hyps))[it] = H;
}

__global__ __launch_bounds__(64 * FT_S3_WAVES) void k_sim3_count(FtSim3SolverCall T) {
    const FtSim3SolverJob *J = (const FtSim3SolverJob *)(T.arena + T.jobs) + blockIdx.y;
    const int it = blockIdx.x * FT_S3_WAVES + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (it >= J->eff) return;  // the whole wave leaves: no barrier below
    const FtSim3Pair *pairs = (const FtSim3Pair *)(T.arena + J->pairs);
    const FtSim3Hyp *H = (const FtSim3Hyp *)(T.arena + J->hyps) + it;
    float T12[12], T21[12];
#pragma unroll
    for (int i = 0; i < 12; i++) T12[i] = H->T12[i], T21[i] = H->T21[i];
    const int N = J->N;
    int count = 0;
    for (int i0 = 0; i0 < N; i0 += 64) {
        const int i = i0 + lane;
        bool in = false;
        if (i < N) in = pair_is_inlier(J, T12, T21, pairs[i]);
        count += __popcll(__ballot(in));
    }
    if (lane == 0) ((int *)(T.arena + J->counts))[it] = count;
}

__global__ __launch_bounds__(256) void k_sim3_select(FtSim3SolverCall T) {
    const FtSim3SolverJob *J = (const FtSim3SolverJob *)(T.arena + T.jobs) + blockIdx.x;
    const int tid = threadIdx.x, eff = J->eff, N = J->N;
    const int *counts = (const int *)(T.arena + J->counts);
    __shared__ int stop, top, best;
    if (tid == 0) stop = eff, top = -1, best = -1;
    __syncthreads();
    for (int k = tid; k < eff; k += 256)
        if (counts[k] > J->minInliers) atomicMin(&stop, k);  // :274
    __syncthreads();
    const bool converged = stop < eff;
    const int last = converged ? stop : eff - 1;
    for (int k = tid; k <= last; k += 256) atomicMax(&top, counts[k]);
    __syncthreads();
    for (int k = tid; k <= last; k += 256)
        if (counts[k] == top) atomicMax(&best, k);  // :265: >= lets a later equal count replace the best
    __syncthreads();
    const int b = best;
    const FtSim3Hyp *H = (const FtSim3Hyp *)(T.arena + J->hyps) + b;
    const FtSim3Pair *pairs = (const FtSim3Pair *)(T.arena + J->pairs);
    float T12[12], T21[12];
#pragma unroll
    for (int i = 0; i < 12; i++) T12[i] = H->T12[i], T21[i] = H->T21[i];
    uint8_t *flags = T.arena + J->flags;
    for (int i = tid; i < N; i += 256) flags[i] = pair_is_inlier(J, T12, T21, pairs[i]) ? 1 : 0;
    if (tid == 0) {
        FtSim3SolverOut *O = (FtSim3SolverOut *)(T.arena + J->out);
        O->converged = converged ? 1 : 0;
        O->iterations = last + 1;
        O->nBest = top;
        O->best = b;
        O->hyp = *H;
    }
}

}  // namespace

int ft_launch_sim3_hypotheses(hipStream_t st, const FtSim3SolverCall &T) {
    hipLaunchKernelGGL(k_sim3_hypotheses, dim3((unsigned)((T.maxEff + 63) / 64), (unsigned)T.nJobs), dim3(64), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_sim3_count(hipStream_t st, const FtSim3SolverCall &T) {
    hipLaunchKernelGGL(k_sim3_count, dim3((unsigned)((T.maxEff + FT_S3_WAVES - 1) / FT_S3_WAVES), (unsigned)T.nJobs), dim3(64 * FT_S3_WAVES), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_sim3_select(hipStream_t st, const FtSim3SolverCall &T) {
    hipLaunchKernelGGL(k_sim3_select, dim3((unsigned)T.nJobs), dim3(256), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

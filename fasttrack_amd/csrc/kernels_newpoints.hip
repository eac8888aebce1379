// HIP kernel of the per-match text of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:483-692) for gfx950
// (wave64): every match of keyframe 1 against every neighbour of a call in one launch, on the match rows where
// ORBmatcher::SearchForTriangulation (kernels_triang.hip) left them.
//   k_triang_points<MODEL>  blockIdx.y = neighbour, blockIdx.x = a chunk of 256 slots of its matches12 row.  A row is sparse (a
//                     keyframe matches a fraction of its features against one neighbour) and a match costs a Newton unprojection,
//                     a 4x4 SVD in double and two projections, so the workgroup first writes status 0 / a zero point for its empty
//                     slots and ballot-compacts the others into an LDS list; lane t then takes entry t of the list: the waves
//                     that run the arithmetic are dense, the others leave at once.
//                     What belongs to the neighbour (its poses, intrinsics, thresholds) is wave-uniform and read from the job
//                     record through the scalar path; a lane selects by its own features only the camera and the pose of a
//                     two-camera keyframe.
//                     n_points[k] and first_neighbour[idx1] are accumulated over workgroups (atomic add per wave, atomic minimum
//                     per accepted point) on the initial values the host stages with the inputs: every other slot is written here.
// Float steps follow the reference's order without contraction (the __f*_rn forms); cos / atan2 of the stereo parallax are cosf /
// atan2f: LocalMapping.cc sees `using namespace std` (LocalMapping.h:23 -> KeyFrame.h:26 -> ORBVocabulary.h:24 ->
// DBoW2/TemplatedVocabulary.h:36), the arguments are floats, so std::cos(float) / std::atan2(float, float) bind, and `min` is
// std::min: (b < a) ? b : a.  The null vector of GeometricTools::Triangulate comes from null_vector4 (see fasttrack_amd.h).
// One instance per camera model, as k_triang_match.
#include "ft_internal.h"
#include "ft_search.h"
#include "kb8_triangulate.h"
#include "wave_ops.h"

namespace {

#define FT_NEWPOINTS_T 256  // threads of a workgroup = slots of a chunk

// pCamera->unprojectEig(kp.pt): Pinhole.cpp:61-64 / KannalaBrandt8.cpp:111-143
template <int MODEL>
__device__ __forceinline__ void unproject(const float *cam, float precision, float px, float py, float r[3]) {
    if (MODEL == 0) {
        r[0] = __fdiv_rn(__fsub_rn(px, cam[2]), cam[0]);
        r[1] = __fdiv_rn(__fsub_rn(py, cam[3]), cam[1]);
        r[2] = 1.f;
    } else {
        kb8_unproject(cam, precision, px, py, r);
    }
}

// pCamera->project(cv::Point3f(x, y, z)): Pinhole.cpp:27-41 / KannalaBrandt8.cpp:43-65
template <int MODEL>
__device__ __forceinline__ void project(const float *cam, const float p[3], float uv[2]) {
    if (MODEL == 0) {
        uv[0] = __fadd_rn(__fdiv_rn(__fmul_rn(cam[0], p[0]), p[2]), cam[2]);
        uv[1] = __fadd_rn(__fdiv_rn(__fmul_rn(cam[1], p[1]), p[2]), cam[3]);
    } else {
        kb8_project(cam, p, uv);
    }
}

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:755-772): mvKeys[i].pt, not the undistorted keypoint
__device__ __forceinline__ bool unproject_stereo(const FtNewPointSide *G, float u, float v, float z, float x3D[3]) {
    if (!(z > 0)) return false;
    const float c[3] = {__fmul_rn(__fmul_rn(__fsub_rn(u, G->cx), z), G->invfx), __fmul_rn(__fmul_rn(__fsub_rn(v, G->cy), z), G->invfy), z};
#pragma unroll
    for (int i = 0; i < 3; i++) x3D[i] = __fadd_rn(fdot3(G->Rwc + 3 * i, c), G->twc[i]);
    return true;
}

// the reprojection test of one keyframe (:621-672): T = its Tcw, (x, y, z) = the point in its camera
template <int MODEL>
__device__ __forceinline__ bool reprojection_fails(bool stereo, const float *cam, const FtNewPointSide *G, float mbf, const float p[3], float kx,
                                                   float ky, float ur, float sigma2) {
    if (!stereo) {
        float uv[2];
        project<MODEL>(cam, p, uv);
        const float ex = __fsub_rn(uv[0], kx), ey = __fsub_rn(uv[1], ky);
        return (double)__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)) > 5.991 * (double)sigma2;
    }
    const float invz = (float)(1.0 / (double)p[2]);
    const float u = __fadd_rn(__fmul_rn(__fmul_rn(G->fx, p[0]), invz), G->cx);
    const float u_r = __fsub_rn(u, __fmul_rn(mbf, invz));
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(G->fy, p[1]), invz), G->cy);
    const float ex = __fsub_rn(u, kx), ey = __fsub_rn(v, ky), er = __fsub_rn(u_r, ur);
    return (double)__fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(er, er)) > 7.8 * (double)sigma2;
}

// one match: -> status, x3D
template <int MODEL>
__device__ int new_point(const uint8_t *arena, const FtTriangCall &T, const FtNewPointCall &P, const FtTriangSide &K2, const FtNewPointSide *G1,
                         const FtNewPointSide *G2, int idx1, int idx2, float x3D[3]) {
    const FtTriangSide &K1 = T.K1;
    const ft_keypoint kp1 = at<ft_keypoint>(arena, K1.keys)[idx1], kp2 = at<ft_keypoint>(arena, K2.keys)[idx2];
    const float ur1 = K1.uright != FT_TRIANG_NONE ? at<float>(arena, K1.uright)[idx1] : -1.f;
    const float ur2 = K2.uright != FT_TRIANG_NONE ? at<float>(arena, K2.uright)[idx2] : -1.f;
    const bool stereo1 = !T.twoCameras && ur1 >= 0, stereo2 = !T.twoCameras && ur2 >= 0;  // :492, :501
    // the pairing ll / lr / rl / rr of two-camera keyframes (:505-555): pose, centre and camera of the feature's own side
    const int s1 = T.twoCameras && K1.nLeft != -1 && idx1 >= K1.nLeft, s2 = T.twoCameras && K2.nLeft != -1 && idx2 >= K2.nLeft;
    const float *T1 = G1->Tcw[s1], *T2 = G2->Tcw[s2];
    const float *cam1 = at<FtTriangSide>(arena, T.k1)->cam[s1], *cam2 = K2.cam[s2];
    float xn1[3], xn2[3], ray1[3], ray2[3];
    unproject<MODEL>(cam1, G1->precision, kp1.x, kp1.y, xn1);
    unproject<MODEL>(cam2, G2->precision, kp2.x, kp2.y, xn2);
#pragma unroll
    for (int i = 0; i < 3; i++) {  // Rwc * xn, Rwc = Rcw.transpose()
        ray1[i] = __fadd_rn(__fmul_rn(T1[i], xn1[0]), __fadd_rn(__fmul_rn(T1[4 + i], xn1[1]), __fmul_rn(T1[8 + i], xn1[2])));
        ray2[i] = __fadd_rn(__fmul_rn(T2[i], xn2[0]), __fadd_rn(__fmul_rn(T2[4 + i], xn2[1]), __fmul_rn(T2[8 + i], xn2[2])));
    }
    const float cosRays = __fdiv_rn(fdot3(ray1, ray2), __fmul_rn(fnorm3(ray1), fnorm3(ray2)));
    const float cosInit = __fadd_rn(cosRays, 1.f);
    float cosStereo1 = cosInit, cosStereo2 = cosInit;
    if (stereo1) cosStereo1 = ft_cos_f(__fmul_rn(2.f, ft_atan2_f(__fdiv_rn(G1->mb, 2.f), at<float>(arena, G1->depth)[idx1])));
    else if (stereo2) cosStereo2 = ft_cos_f(__fmul_rn(2.f, ft_atan2_f(__fdiv_rn(G2->mb, 2.f), at<float>(arena, G2->depth)[idx2])));
    const float cosStereo = cosStereo2 < cosStereo1 ? cosStereo2 : cosStereo1;  // std::min(cosParallaxStereo1, cosParallaxStereo2)
    int ok;
    if (cosRays < cosStereo && cosRays > 0 &&
        (stereo1 || stereo2 || ((double)cosRays < 0.9996 && P.inertial) || ((double)cosRays < 0.9998 && !P.inertial))) {
        // GeometricTools::Triangulate (src/GeometricTools.cc:47-66)
        double A[16], v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            A[j] = (double)__fsub_rn(__fmul_rn(xn1[0], T1[8 + j]), T1[j]);
            A[4 + j] = (double)__fsub_rn(__fmul_rn(xn1[1], T1[8 + j]), T1[4 + j]);
            A[8 + j] = (double)__fsub_rn(__fmul_rn(xn2[0], T2[8 + j]), T2[j]);
            A[12 + j] = (double)__fsub_rn(__fmul_rn(xn2[1], T2[8 + j]), T2[4 + j]);
        }
        null_vector4(A, v);
        const float w = (float)v[3];
        if (w == 0) return -2;
#pragma unroll
        for (int i = 0; i < 3; i++) x3D[i] = __fdiv_rn((float)v[i], w);
        ok = 1;
    } else if (stereo1 && cosStereo1 < cosStereo2) {
        const ft_keypoint raw = at<ft_keypoint>(arena, G1->keysRaw != FT_TRIANG_NONE ? G1->keysRaw : K1.keys)[idx1];
        if (!unproject_stereo(G1, raw.x, raw.y, at<float>(arena, G1->depth)[idx1], x3D)) return -2;
        ok = 2;
    } else if (stereo2 && cosStereo2 < cosStereo1) {
        const ft_keypoint raw = at<ft_keypoint>(arena, G2->keysRaw != FT_TRIANG_NONE ? G2->keysRaw : K2.keys)[idx2];
        if (!unproject_stereo(G2, raw.x, raw.y, at<float>(arena, G2->depth)[idx2], x3D)) return -2;
        ok = 3;
    } else {
        return -1;  // no stereo and very low parallax (:603)
    }
    const float z1 = __fadd_rn(fdot3(T1 + 8, x3D), T1[11]);
    if (z1 <= 0) return -3;
    const float z2 = __fadd_rn(fdot3(T2 + 8, x3D), T2[11]);
    if (z2 <= 0) return -4;
    const float p1[3] = {__fadd_rn(fdot3(T1, x3D), T1[3]), __fadd_rn(fdot3(T1 + 4, x3D), T1[7]), z1};
    if (reprojection_fails<MODEL>(stereo1, cam1, G1, G1->mbf, p1, kp1.x, kp1.y, ur1, at<float>(arena, K1.sigma2)[kp1.octave])) return -5;
    const float p2[3] = {__fadd_rn(fdot3(T2, x3D), T2[3]), __fadd_rn(fdot3(T2 + 4, x3D), T2[7]), z2};
    // :665 subtracts mpCurrentKeyFrame->mbf * invz2: keyframe 1's mbf in keyframe 2's test
    if (reprojection_fails<MODEL>(stereo2, cam2, G2, G1->mbf, p2, kp2.x, kp2.y, ur2, at<float>(arena, K2.sigma2)[kp2.octave])) return -6;
    const float *Ow1 = G1->Ow[s1], *Ow2 = G2->Ow[s2];
    const float n1[3] = {__fsub_rn(x3D[0], Ow1[0]), __fsub_rn(x3D[1], Ow1[1]), __fsub_rn(x3D[2], Ow1[2])};
    const float n2[3] = {__fsub_rn(x3D[0], Ow2[0]), __fsub_rn(x3D[1], Ow2[1]), __fsub_rn(x3D[2], Ow2[2])};
    const float dist1 = fnorm3(n1), dist2 = fnorm3(n2);
    if (dist1 == 0 || dist2 == 0) return -7;
    if (P.farPoints && (dist1 >= P.thFar || dist2 >= P.thFar)) return -8;
    const float ratioDist = __fdiv_rn(dist2, dist1);
    const float ratioOctave = __fdiv_rn(at<float>(arena, K1.sf)[kp1.octave], at<float>(arena, K2.sf)[kp2.octave]);
    if (__fmul_rn(ratioDist, P.ratioFactor) < ratioOctave || ratioDist > __fmul_rn(ratioOctave, P.ratioFactor)) return -9;
    return ok;
}

template <int MODEL>  // 0 pinhole, 1 KannalaBrandt8
__global__ __launch_bounds__(FT_NEWPOINTS_T) void k_triang_points(FtTriangCall T, FtNewPointCall P) {
    __shared__ int list[FT_NEWPOINTS_T];
    __shared__ int waveCount[FT_NEWPOINTS_T / 64];
    uint8_t *arena = T.arena;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.y, n1 = T.K1.fv.n;
    const int base = (int)blockIdx.x * FT_NEWPOINTS_T;
    const FtTriangJob *job = at<FtTriangJob>(arena, T.jobs) + k;
    const FtNewPointJob *nj = at<FtNewPointJob>(arena, P.jobs) + k;
    const int *matches = at<int>(arena, job->matches);
    int *status = (int *)(arena + nj->status);
    float *x3d = (float *)(arena + nj->x3d);
    const int slot = base + tid;
    const bool has = slot < n1 && matches[slot] >= 0;
    if (slot < n1 && !has) {
        status[slot] = 0;
        x3d[3 * (size_t)slot] = 0.f;
        x3d[3 * (size_t)slot + 1] = 0.f;
        x3d[3 * (size_t)slot + 2] = 0.f;
    }
    const unsigned long long mask = __ballot(has);
    if (lane == 0) waveCount[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < FT_NEWPOINTS_T / 64; w++) {
        const int c = waveCount[w];
        before += w < wave ? c : 0;
        total += c;
    }
    if (has) list[before + __popcll(mask & ((1ull << lane) - 1ull))] = tid;
    __syncthreads();
    if (wave * 64 >= total) return;  // the whole wave: nothing behind this point is a workgroup barrier
    bool accepted = false;
    if (tid < total) {
        const int idx1 = base + list[tid];
        const int idx2 = matches[idx1];
        float p[3] = {0.f, 0.f, 0.f};
        const FtNewPointSide *G1 = at<FtNewPointSide>(arena, P.g1);
        const int st = new_point<MODEL>(arena, T, P, job->K2, G1, &nj->G2, idx1, idx2, p);
        accepted = st > 0;
        status[idx1] = st;
        x3d[3 * (size_t)idx1] = accepted ? p[0] : 0.f;
        x3d[3 * (size_t)idx1 + 1] = accepted ? p[1] : 0.f;
        x3d[3 * (size_t)idx1 + 2] = accepted ? p[2] : 0.f;
        if (accepted) atomicMin((unsigned *)(arena + P.firstNeighbour) + idx1, (unsigned)k);
    }
    const int cnt = __popcll(__ballot(accepted));
    if (lane == 0 && cnt) atomicAdd((int *)(arena + P.nPoints) + k, cnt);
}

}  // namespace

int ft_launch_triang_points(hipStream_t st, const FtTriangCall &T, const FtNewPointCall &P) {
    const dim3 grid((T.K1.fv.n + FT_NEWPOINTS_T - 1) / FT_NEWPOINTS_T, T.nNeighbours);
    if (T.camModel == 0) hipLaunchKernelGGL(k_triang_points<0>, grid, dim3(FT_NEWPOINTS_T), 0, st, T, P);
    else hipLaunchKernelGGL(k_triang_points<1>, grid, dim3(FT_NEWPOINTS_T), 0, st, T, P);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

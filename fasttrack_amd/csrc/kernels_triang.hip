// HIP kernels of ORBmatcher::SearchForTriangulation (reference src/ORBmatcher.cc:1006-1245) for gfx950 (wave64): keyframe 1
// against every neighbour of a call (LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:388-466), two launches whatever the
// number of neighbours.
//   k_triang_match<MODEL>  blockIdx.y = neighbour.  A row of 16 lanes per feature of keyframe 1 (four features per wave): the
//                     row finds the feature's vocabulary node on the neighbour's side by binary search (the reference's
//                     lower_bound walk visits exactly the common keys), its lanes take the node's candidates 16 at a time and
//                     apply the whole eligibility test to theirs - map point, stereo, TH_LOW, epipole, epipolar constraint -,
//                     the minimum key (dist << 20 | 0xFFFFF - position) of the row is the match: the smallest distance, among
//                     equals the LAST of the node's list (the reference's scan skips on dist > bestDist, :1116, so an equal
//                     distance replaces).  vbMatched2 is never written in the reference (:1048, :1103): no feature sees what
//                     another one chose, every row is independent.  The constraint is a pure function, so evaluating it for
//                     every candidate with dist <= TH_LOW instead of in the reference's lazy order changes nothing.
//                     One instance per camera model: the pinhole one does not carry the registers of the double-precision SVD.
//   k_triang_finish   a workgroup per neighbour: rotation histogram over the matches (:1186-1196), ComputeThreeMaxima, the
//                     removal (:1213-1232), nmatches.
// A row and not a wave per feature: with levelsup 4 of a 10^6-word tree a node holds tens of features (2 000 features over
// ~100 nodes), so a wave of 64 candidates would idle two thirds of its lanes.
#include <algorithm>

#include "ft_internal.h"
#include "ft_search.h"
#include "kb8_triangulate.h"
#include "rot_filter_dev.h"
#include "wave_ops.h"

namespace {

#define FT_TRIANG_T 256                    // threads of a k_triang_match workgroup
#define FT_TRIANG_ROWS (FT_TRIANG_T / 16)  // features of keyframe 1 per workgroup
#define FT_TRIANG_FIN_T 256

// Pinhole::epipolarConstrain (src/CameraModels/Pinhole.cpp:107-129) behind the line [a b c] = x1' F12 of the feature
__device__ __forceinline__ bool pinhole_constrain(float a, float b, float c, float x2, float y2, float unc) {
    const float num = __fadd_rn(__fadd_rn(__fmul_rn(a, x2), __fmul_rn(b, y2)), c);
    const float den = __fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b));
    if (den == 0.f) return false;
    const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
    return (double)dsqr < 3.84 * (double)unc;
}

template <int MODEL>  // 0 pinhole, 1 KannalaBrandt8
__global__ __launch_bounds__(FT_TRIANG_T) void k_triang_match(FtTriangCall T) {
    const uint8_t *arena = T.arena;
    const int sub = threadIdx.x & 15;
    const int idx1 = (int)blockIdx.x * FT_TRIANG_ROWS + (int)(threadIdx.x >> 4);
    const FtTriangJob *job = at<FtTriangJob>(arena, T.jobs) + blockIdx.y;
    const FtTriangSide &K1 = T.K1;
    const FtTriangSide &K2 = job->K2;
    constexpr unsigned NONE = 0xffffffffu;
    unsigned best = NONE;
    const bool live = idx1 < K1.fv.n;
    // every lane of a row takes the same way through the tests of the feature: the row stays whole for its reduction
    int a1 = live ? at<int>(arena, T.nodeOf)[idx1] : -1;
    if (a1 >= 0 && at<uint8_t>(arena, K1.hasPoint)[idx1]) a1 = -1;  // pMP1 (:1073)
    bool stereo1 = false;
    if (a1 >= 0) {
        stereo1 = !T.twoCameras && K1.uright != FT_TRIANG_NONE && at<float>(arena, K1.uright)[idx1] >= 0.f;  // :1078
        if (T.onlyStereo && !stereo1) a1 = -1;
    }
    int fBeg = 0, fCnt = 0;
    if (a1 >= 0) {
        const int lo = fv_find_node(at<unsigned>(arena, K2.fv.nodes), K2.fv.nNodes, at<unsigned>(arena, K1.fv.nodes)[a1]);
        if (lo >= 0) {
            const int *offs2 = at<int>(arena, K2.fv.offsets);
            fBeg = offs2[lo];
            fCnt = offs2[lo + 1] - fBeg;
        }
    }
    if (fCnt > 0) {
        const ft_keypoint kp1 = at<ft_keypoint>(arena, K1.keys)[idx1];
        const bool right1 = K1.nLeft != -1 && idx1 >= K1.nLeft;  // :1088
        unsigned long long d1[4];
        {
            const unsigned long long *p = at<unsigned long long>(arena, K1.desc) + (size_t)idx1 * 4;
            d1[0] = p[0]; d1[1] = p[1]; d1[2] = p[2]; d1[3] = p[3];
        }
        const float sigma1 = at<float>(arena, K1.sigma2)[kp1.octave];
        float la = 0.f, lb = 0.f, lc = 0.f;
        if (MODEL == 0) {  // l = x1' F12 (Pinhole.cpp:115-117)
            const float *F = job->F12;
            la = __fadd_rn(__fadd_rn(__fmul_rn(kp1.x, F[0]), __fmul_rn(kp1.y, F[3])), F[6]);
            lb = __fadd_rn(__fadd_rn(__fmul_rn(kp1.x, F[1]), __fmul_rn(kp1.y, F[4])), F[7]);
            lc = __fadd_rn(__fadd_rn(__fmul_rn(kp1.x, F[2]), __fmul_rn(kp1.y, F[5])), F[8]);
        }
        const unsigned *feats2 = at<unsigned>(arena, K2.fv.feats) + fBeg;
        const uint8_t *has2 = at<uint8_t>(arena, K2.hasPoint);
        const ft_keypoint *keys2 = at<ft_keypoint>(arena, K2.keys);
        for (int p = sub; p < fCnt; p += 16) {
            const int idx2 = (int)feats2[p];
            if (has2[idx2]) continue;  // pMP2 (:1103; vbMatched2 is all false)
            const bool stereo2 = !T.twoCameras && K2.uright != FT_TRIANG_NONE && at<float>(arena, K2.uright)[idx2] >= 0.f;  // :1106
            if (T.onlyStereo && !stereo2) continue;
            const int dist = hamming256(d1, at<unsigned long long>(arena, K2.desc) + (size_t)idx2 * 4);
            if (dist > FT_TH_LOW) continue;  // :1116
            const ft_keypoint kp2 = keys2[idx2];
            if (!stereo1 && !stereo2 && !T.twoCameras) {  // :1125-1133
                const float distex = __fsub_rn(job->ep[0], kp2.x), distey = __fsub_rn(job->ep[1], kp2.y);
                if (__fadd_rn(__fmul_rn(distex, distex), __fmul_rn(distey, distey)) < __fmul_rn(100.f, at<float>(arena, K2.sf)[kp2.octave]))
                    continue;
            }
            if (!T.coarse) {  // :1171
                const float sigma2 = at<float>(arena, K2.sigma2)[kp2.octave];
                bool ok;
                if (MODEL == 0) {
                    ok = pinhole_constrain(la, lb, lc, kp2.x, kp2.y, sigma2);
                } else {
                    const bool right2 = K2.nLeft != -1 && idx2 >= K2.nLeft;
                    // the pairing ll, lr, rl, rr of two-camera keyframes (:1135-1169); T12 with the first cameras otherwise
                    const int pairing = T.twoCameras ? (right1 ? 2 : 0) + (right2 ? 1 : 0) : 0;
                    const float *c1 = at<FtTriangSide>(arena, T.k1)->cam[T.twoCameras && right1 ? 1 : 0], *c2 = K2.cam[T.twoCameras && right2 ? 1 : 0];
                    float p3[3];
                    ok = kb8_triangulate_matches(c1, c2, job->precision, job->R12[pairing], job->t12[pairing], kp1.x, kp1.y, kp2.x, kp2.y,
                                                 sigma1, sigma2, p3) > 0.0001f;
                }
                if (!ok) continue;
            }
            best = min(best, ((unsigned)dist << 20) | (0xfffffu - (unsigned)p));
        }
    }
    best = row_min_u32(best);
    if (live && sub == 0) {
        int m = -1, bd = FT_TH_LOW;
        if (best != NONE) {
            bd = (int)(best >> 20);
            m = (int)at<unsigned>(arena, K2.fv.feats)[fBeg + (int)(0xfffffu - (best & 0xfffffu))];
        }
        ((int *)(arena + job->matches))[idx1] = m;
        ((int *)(arena + job->bestDist))[idx1] = bd;
    }
}

__global__ __launch_bounds__(FT_TRIANG_FIN_T) void k_triang_finish(FtTriangCall T) {
    uint8_t *arena = T.arena;
    const FtTriangJob *job = at<FtTriangJob>(arena, T.jobs) + blockIdx.x;
    const ft_keypoint *keys1 = at<ft_keypoint>(arena, T.K1.keys), *keys2 = at<ft_keypoint>(arena, job->K2.keys);
    // kp1.angle - kp2.angle (:1188); the removal :1221-1230
    rot_filter_rows<FT_TRIANG_FIN_T>((int *)(arena + job->matches), T.K1.fv.n, T.checkOrientation, (int *)(arena + T.nMatches) + blockIdx.x,
                                     [&](int i, int m) { return init_bin(keys1[i].angle, keys2[m].angle); });
}

}  // namespace

int ft_launch_triang_match(hipStream_t st, const FtTriangCall &T) {
    const dim3 grid((T.K1.fv.n + FT_TRIANG_ROWS - 1) / FT_TRIANG_ROWS, T.nNeighbours);
    if (T.camModel == 0) hipLaunchKernelGGL(k_triang_match<0>, grid, dim3(FT_TRIANG_T), 0, st, T);
    else hipLaunchKernelGGL(k_triang_match<1>, grid, dim3(FT_TRIANG_T), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_triang_finish(hipStream_t st, const FtTriangCall &T) {
    hipLaunchKernelGGL(k_triang_finish, dim3(T.nNeighbours), dim3(FT_TRIANG_FIN_T), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

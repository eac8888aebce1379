// HIP kernels of the relocalisation matcher for gfx950 (wave64):
//   ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist)   (reference src/ORBmatcher.cc:2087-2208)
//
// The reference walks the keyframe's map points in index order; a point takes the nearest keypoint of its window whose
// mvpMapPoints entry is still NULL - held before the call (whatever its Observations()) or written by an earlier point of
// this call - and writes it when the distance is <= ORBdist.  Windows, level bands and distances do not depend on that
// state, the choice does, so the work is split as in kernels_init.hip (the terms POINT and key: ft_search.h):
//   k_reloc_project     a thread per point: Tcw * x3Dw in the Sophus form, the camera model, the image bounds (NO depth
//                       test: :2112-2119), the distance to Ow = Tcw.inverse().translation() against the point's range,
//                       PredictScale - the record {u, v, level, go}
//   k_reloc_candidates  a wave per point: the window GetFeaturesInArea(u, v, th * sf[level], level - 1, level + 1) of the
//                       LEFT camera in the per-octave grid; the keypoints that are not held on entry, as keys
//                       (distance, cell x, cell y, index), into the point's segment, the FT_RELOC_TOP smallest in front
//   k_reloc_resolve     one workgroup: the sequential part.  A taken bit per keypoint in LDS; wave 0 walks the points in
//                       order and gives each its smallest key whose keypoint is free (strict < of :2157 = the first of equal
//                       distances in GetFeaturesInArea's order = the smallest key) - from the top record unless all of it
//                       is taken and the segment holds more.  Then, by the whole workgroup: rotation histogram,
//                       ComputeThreeMaxima, the removal, nmatches, assign and holder_obs.
// Three launches per call, whatever the inputs hold.
#include <algorithm>

#include "rot_filter_dev.h"
#include "search_dev.h"

namespace {

#define FT_RELOC_WPB 4

__global__ __launch_bounds__(256) void k_reloc_project(FtRelocSearch S) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S.N) return;
    const FtDevFrame &F = S.F;
    FtRelocProj pj;
    pj.u = 0.f;
    pj.v = 0.f;
    pj.level = 0;
    pj.go = 0;
    if (S.valid[i]) {
        const float xw[3] = {S.worldPos[3 * i], S.worldPos[3 * i + 1], S.worldPos[3 * i + 2]};
        float xc[3], uv[2];
        transform_pose(S.Tcw.m, S.Tcw.q, 1, xw, xc);
        project_cam(F, xc, uv);
        // :2116-2119 as written (a NaN - x3Dc.z == 0 - passes them in the reference and is undefined from there on: dropped here)
        bool go = !(uv[0] < F.mnMinX || uv[0] > F.mnMaxX) && !(uv[1] < F.mnMinY || uv[1] > F.mnMaxY);
        go = go && uv[0] == uv[0] && uv[1] == uv[1];
        if (go) {
            // Ow = Tcw.inverse().translation() (:2092; se3.hpp: so3().inverse() * (translation() * -1)): the conjugate quaternion
            // applied to -t as every rotation is applied to a point
            const float zero[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const float qc[4] = {-S.Tcw.q[0], -S.Tcw.q[1], -S.Tcw.q[2], S.Tcw.q[3]};
            const float nt[3] = {-S.Tcw.m[3], -S.Tcw.m[7], -S.Tcw.m[11]};
            float Ow[3];
            transform_pose(zero, qc, 1, nt, Ow);
            const float PO[3] = {__fsub_rn(xw[0], Ow[0]), __fsub_rn(xw[1], Ow[1]), __fsub_rn(xw[2], Ow[2])};
            const float dist3D = norm3(PO);
            const float maxRaw = S.maxDist[i];
            const float maxDistance = __fmul_rn(1.2f, maxRaw), minDistance = __fmul_rn(0.8f, S.minDist[i]);
            if (dist3D < minDistance || dist3D > maxDistance) go = false;
            if (go) {
                pj.u = uv[0];
                pj.v = uv[1];
                pj.level = predict_scale(maxRaw, dist3D, S.logScaleFactor, F.nlevels);
            }
        }
        pj.go = go ? 1 : 0;
    }
    S.proj[i] = pj;
}

__global__ __launch_bounds__(64 * FT_RELOC_WPB) void k_reloc_candidates(FtRelocSearch S) {
    __shared__ int counter[FT_RELOC_WPB];
    const int lane = threadIdx.x & 63, wave = wave_index();
    const int i = (int)blockIdx.x * FT_RELOC_WPB + wave;
    if (i >= S.N) return;
    const FtDevFrame &F = S.F;
    const FramePtrs Q = frame_ptrs(F, FT_NO_REBASE);
    const FtRelocProj pj = S.proj[i];
    unsigned long long t[FT_RELOC_TOP];
#pragma unroll
    for (int k = 0; k < FT_RELOC_TOP; k++) t[k] = KEY_NONE;
    int count = 0;
    if (__builtin_amdgcn_readfirstlane(pj.go)) {
        const int level = __builtin_amdgcn_readfirstlane(pj.level);
        const float u = pj.u, v = pj.v;
        const float radius = __fmul_rn(S.th, F.sf[level]);
        const Window w = cell_window(F, u, v, radius);
        if (!w.empty) {
            unsigned long long d1[4];
            load_desc256(S.desc, i, d1);
            unsigned long long *seg = S.seg + (size_t)i * FT_RELOC_SEG;
            int *ctr = &counter[wave];
            if (lane == 0) *ctr = 0;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int nLeft = F.Nleft == -1 ? F.N : F.Nleft;
            for_window(F, Q, 0, Q.keys, nLeft, w, level - 1, level + 1, lane, [&](const WinEntry &kp) {
                if (!in_box(kp, u, v, radius, level - 1, level + 1)) return;
                if (S.holder[kp.idx] != -1) return;  // CurrentFrame.mvpMapPoints[i2] (:2150), whatever its Observations()
                const unsigned long long key = make_key(hamming256(d1, kp.d), kp.cx, kp.cy, kp.idx, kp.octave, false);
                const int at = atomicAdd(ctr, 1);
                if (at < FT_RELOC_SEG) seg[at] = key;
                top_insert<FT_RELOC_TOP>(t, key);
            });
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            count = *ctr;
        }
    }
    // the FT_RELOC_TOP smallest keys of the wave: the lanes' lists are ascending, so the wave's minimum is some lane's head
    unsigned long long out = KEY_NONE;
#pragma unroll
    for (int k = 0; k < FT_RELOC_TOP; k++) {
        const unsigned long long m = wave_min_u64(t[0]);
        if (lane == k) out = m;
        if (t[0] == m && m != KEY_NONE) {  // (keys are unique inside a window: one lane pops)
#pragma unroll
            for (int j = 0; j + 1 < FT_RELOC_TOP; j++) t[j] = t[j + 1];
            t[FT_RELOC_TOP - 1] = KEY_NONE;
        }
    }
    if (lane < FT_RELOC_TOP) S.top[(size_t)i * FT_RELOC_TOP + lane] = out;
    if (lane == 0) {
        S.segCount[i] = min(count, FT_RELOC_SEG);
        if (count > FT_RELOC_SEG) atomicOr(S.status, 1);
    }
}

// LDS: taken[kp >> 5] bit kp & 31 = mvpMapPoints[kp] was written by an earlier point of this call (the keypoints held on
// entry never became candidates), then match[i] = the keypoint point i wrote, -1 = none.
#define FT_RELOC_RES_T 1024
__global__ __launch_bounds__(FT_RELOC_RES_T) void k_reloc_resolve(FtRelocSearch S) {
    extern __shared__ unsigned rel_lds[];
    __shared__ int rel_nm;
    const int tid = threadIdx.x, lane = tid & 63;
    const FtDevFrame &F = S.F;
    const int nLeft = F.Nleft == -1 ? F.N : F.Nleft;
    const int nWords = (nLeft + 31) / 32;
    if (__builtin_amdgcn_readfirstlane(S.status[0]) != 0) return;  // a truncated candidate list: nothing is written
    unsigned *taken = rel_lds;
    int *match = (int *)(rel_lds + nWords);
    for (int k = tid; k < nWords; k += FT_RELOC_RES_T) taken[k] = 0u;
    if (tid == 0) rel_nm = 0;
    for (int k = tid; k < F.N; k += FT_RELOC_RES_T) S.assign[k] = -1;
    __threadfence();
    __syncthreads();
    const int N = S.N;
    if (tid < 64) {  // the sequential walk over the points, wave 0; every decision below is wave-uniform
        const uint4 *top4 = (const uint4 *)S.top;  // FT_RELOC_TOP keys = two 16-byte words per point
        uint4 nextA = make_uint4(~0u, ~0u, ~0u, ~0u), nextB = nextA;
        int nextCnt = 0;
        if (lane < N) {
            nextA = top4[2 * (size_t)lane];
            nextB = top4[2 * (size_t)lane + 1];
            nextCnt = S.segCount[lane];
        }
        for (int r0 = 0; r0 < N; r0 += 64) {
            const uint4 curA = nextA, curB = nextB;
            const int curCnt = nextCnt;
            if (r0 + 64 + lane < N) {  // the next 64 points are on their way while these are decided
                nextA = top4[2 * (size_t)(r0 + 64 + lane)];
                nextB = top4[2 * (size_t)(r0 + 64 + lane) + 1];
                nextCnt = S.segCount[r0 + 64 + lane];
            }
            const int nr = min(64, N - r0);
            int myDist = 256, myIdx = -1, myMatch = -1;  // lane j: the outcome of point r0 + j
            for (int j = 0; j < nr; j++) {
                const int cnt = __builtin_amdgcn_readlane(curCnt, j);
                if (cnt <= 0) continue;  // not searched, or no free candidate in its window
                auto key_of = [&](unsigned lo, unsigned hi) {
                    return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hi, j) << 32) |
                           (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)lo, j);
                };
                const unsigned long long k[FT_RELOC_TOP] = {key_of(curA.x, curA.y), key_of(curA.z, curA.w), key_of(curB.x, curB.y),
                                                            key_of(curB.z, curB.w)};
                unsigned long long best = KEY_NONE;
#pragma unroll
                for (int q = FT_RELOC_TOP - 1; q >= 0; q--) {
                    if (k[q] == KEY_NONE) continue;
                    const int kp = min(key_idx(k[q]), nLeft - 1);
                    const bool free_ = ((taken[kp >> 5] >> (kp & 31)) & 1u) == 0u;
                    if (free_) best = k[q];  // (descending q: the smallest free key stays)
                }
                if (best == KEY_NONE && cnt > FT_RELOC_TOP) {  // all of the top record is taken and the window holds more
                    const unsigned long long *seg = S.seg + (size_t)(r0 + j) * FT_RELOC_SEG;
                    unsigned long long k0 = KEY_NONE;
                    for (int e = lane; e < cnt; e += 64) {
                        const unsigned long long key = seg[e];
                        const int kp = min(key_idx(key), nLeft - 1);
                        if ((taken[kp >> 5] >> (kp & 31)) & 1u) continue;
                        k0 = key < k0 ? key : k0;
                    }
                    best = wave_min_u64(k0);
                }
                if (best == KEY_NONE) continue;
                const int bd = key_dist(best), bi = min(key_idx(best), nLeft - 1);
                const bool accept = bd <= S.orbDist;  // :2164
                if (lane == j) {
                    myDist = bd;
                    myIdx = bi;
                    myMatch = accept ? bi : -1;
                }
                if (accept && lane == 0) taken[bi >> 5] |= 1u << (bi & 31);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if (lane < nr) {
                match[r0 + lane] = myMatch;
                if (S.bestDist) S.bestDist[r0 + lane] = myDist;
                if (S.bestIdx) S.bestIdx[r0 + lane] = myIdx;
            }
        }
    }
    __syncthreads();
    // pKF->mvKeysUn[i].angle - CurrentFrame.mvKeysUn[bestIdx2].angle (:2171)
    auto bin_of = [&](int i, int m) { return init_bin(S.angle[i], F.keys[m].angle); };
    const int keep = rot_filter_keep<FT_RELOC_RES_T>(N, S.checkOrientation, [&](int i) {
        const int m = match[i];
        return m < 0 ? -1 : bin_of(i, m);
    });
    int nm = 0;
    for (int i = tid; i < N; i += FT_RELOC_RES_T) {
        const int m = match[i];
        if (m < 0) continue;
        if (S.checkOrientation) {
            const int bin = bin_of(i, m);
            if (bin >= 0 && bin < FT_HISTO_LENGTH && !((keep >> bin) & 1)) continue;  // removed (:2194-2204): the entry is NULL again
        }
        S.assign[m] = i;
        S.holder[m] = S.obs[i];
        nm++;
    }
    nm = wave_sum_i32(nm);
    if (lane == 0 && nm) atomicAdd(&rel_nm, nm);
    __syncthreads();
    if (tid == 0) *S.nMatches = rel_nm;
}

}  // namespace

int ft_launch_reloc_project(hipStream_t st, const FtRelocSearch &S) {
    hipLaunchKernelGGL(k_reloc_project, dim3(std::max(1, (S.N + 255) / 256)), dim3(256), 0, st, S);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_reloc_candidates(hipStream_t st, const FtRelocSearch &S) {
    hipLaunchKernelGGL(k_reloc_candidates, dim3(std::max(1, (S.N + FT_RELOC_WPB - 1) / FT_RELOC_WPB)), dim3(64 * FT_RELOC_WPB), 0, st, S);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_reloc_resolve(hipStream_t st, const FtRelocSearch &S) {
    const size_t lds = ft_reloc_lds_bytes(S.F.Nleft == -1 ? S.F.N : S.F.Nleft, S.N);
    if (lds > FT_INIT_MAX_LDS) {
        ft_set_error("SearchByProjection(Frame, KeyFrame): keypoints and points exceed the LDS tables of the resolution");
        return FT_ERR_CAPACITY;
    }
    const int rc = ft_allow_max_lds<k_reloc_resolve>();
    if (rc != FT_OK) return rc;
    hipLaunchKernelGGL(k_reloc_resolve, dim3(1), dim3(FT_RELOC_RES_T), lds, st, S);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

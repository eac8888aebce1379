// HIP kernels that prepare a frame for the projection searches and deliver their results (gfx950, wave64):
//   k_build_grid(_batch)       Frame::AssignFeaturesToGrid (reference src/Frame.cc:409-440) as one CSR per octave
//   k_frustum(_batch)          Frame::isInFrustum / isInFrustumChecks (src/Frame.cc:536-610, 1308-1382) + MapPoint::PredictScale
//   k_fill_*                   the start values of a claim iteration
//   k_gather_batch, k_deliver_blocks, k_deliver_batch   pinned host memory <-> device, one launch per direction
// The searches themselves: kernels_search.hip, kernels_search_rows.hip, kernels_resolve.hip.  The two-camera frames of a batch
// from what two extractors left in HBM (ft_tracked_batch_bind_fisheye): kernels_fisheye.hip.
#include <algorithm>

#include "search_dev.h"
#include "libm_f32.h"

namespace {

// (build_grid_body, the counting sort of one (octave, camera) of a frame: search_dev.h - kernels_fuse.hip files the views of a call with it)
__global__ __launch_bounds__(256) void k_build_grid(FtDevFrame F, int *startL, int *startR, float4 *recL, uint8_t *descL, float4 *recR,
                                                    uint8_t *descR) {
    build_grid_body(F, frame_ptrs(F, FT_NO_REBASE), blockIdx.x, blockIdx.y, startL, startR, recL, descL, recR, descR);
}
// the grids of the frames of a batch (ft_tracked_batch): blockIdx.z = frame; the arrays are those F.gridStart / gridRec /
// gridDesc of the frame's job already point to
__global__ __launch_bounds__(256) void k_build_grid_batch(const FtBatchJob *__restrict__ jobs, Rebase rb) {
    const FtDevFrame &F = jobs[blockIdx.z].F;
    if ((int)blockIdx.x >= F.nlevels || (blockIdx.y == 1 && F.Nleft == -1)) return;
    const FramePtrs Q = frame_ptrs(F, rb);
    build_grid_body(F, Q, blockIdx.x, blockIdx.y, (int *)Q.gridStart[0], (int *)Q.gridStart[1], (float4 *)Q.gridRec[0],
                    (uint8_t *)Q.gridDesc[0], (float4 *)Q.gridRec[1], (uint8_t *)Q.gridDesc[1]);
}

// ------------------------------------------------------------------------------------------------
// Frame::isInFrustum / isInFrustumChecks (src/Frame.cc:536-610, 1308-1382) with MapPoint::PredictScale
// (src/MapPoint.cc:531-546): one thread per local map point.  Float expressions are evaluated in the
// order the oracle states (no contraction); log(ratio) binds to logf (MapPoint.cc:539), reproduced by libm_f32.h.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void frustum_point(const FtDevFrame &F, const FtFrustumPose &T, const FtDevMapPoints &P, float viewingCosLimit,
                                              float logScaleFactor, int farPoints, float thFar, const FtFrustumOut &O, int i) {
    if (i >= P.M) return;
    bool inView = false, inViewR = false;
    int level = -1, levelR = -1;
    float viewCosL = 0.f, viewCosR = 0.f, px = -1.f, py = -1.f, pxr = -1.f, pyr = -1.f, depth = 0.f, depthR = 0.f;
    if (!(P.skip && P.skip[i])) {
        const float Pw[3] = {P.worldPos[3 * i], P.worldPos[3 * i + 1], P.worldPos[3 * i + 2]};
        const float Pn[3] = {P.normal[3 * i], P.normal[3 * i + 1], P.normal[3 * i + 2]};
        const float maxRaw = P.maxDist[i];
        const float maxDistance = __fmul_rn(1.2f, maxRaw), minDistance = __fmul_rn(0.8f, P.minDist[i]);
        const int nCams = F.Nleft == -1 ? 1 : 2;
        for (int cam = 0; cam < nCams; cam++) {
            float Pc[3];
#pragma unroll
            for (int r = 0; r < 3; r++) Pc[r] = __fadd_rn(dot3(T.R[cam] + 3 * r, Pw), T.t[cam][r]);
            const float PcDist = norm3(Pc);
            if (Pc[2] < 0.0f) continue;
            float uv[2];
            project_cam(F, Pc, uv);
            if (uv[0] < F.mnMinX || uv[0] > F.mnMaxX) continue;
            if (uv[1] < F.mnMinY || uv[1] > F.mnMaxY) continue;
            if (F.Nleft == -1) {  // Frame.cc:564-565: set before the remaining checks
                px = uv[0];
                py = uv[1];
            }
            const float PO[3] = {__fsub_rn(Pw[0], T.twc[cam][0]), __fsub_rn(Pw[1], T.twc[cam][1]), __fsub_rn(Pw[2], T.twc[cam][2])};
            const float dist = norm3(PO);
            if (dist < minDistance || dist > maxDistance) continue;
            const float viewCos = __fdiv_rn(dot3(PO, Pn), dist);
            if (viewCos < viewingCosLimit) continue;
            const int lv = predict_scale(maxRaw, dist, logScaleFactor, F.nlevels);
            if (cam == 0) {
                inView = true;
                px = uv[0];
                py = uv[1];
                level = lv;
                viewCosL = viewCos;
                depth = PcDist;
                if (F.Nleft == -1) pxr = __fsub_rn(uv[0], __fmul_rn(F.mbf, __fdiv_rn(1.0f, Pc[2])));  // mTrackProjXR (:587)
            } else {
                inViewR = true;
                pxr = uv[0];
                pyr = uv[1];
                levelR = lv;
                viewCosR = viewCos;
                depthR = PcDist;
            }
        }
    }
    O.inView[i] = inView;
    O.inViewR[i] = inViewR;
    O.level[i] = level;
    O.levelR[i] = levelR;
    O.viewCos[i] = viewCosL;
    O.viewCosR[i] = viewCosR;
    O.projX[i] = px;
    O.projY[i] = py;
    O.projXR[i] = pxr;
    O.projYR[i] = pyr;
    O.depth[i] = depth;
    O.depthR[i] = depthR;
    // ORBmatcher.cc:66-74: not in view of either camera, or farther than thFarPoints (the caller's skip holds isBad())
    if (O.searchSkip)
        O.searchSkip[i] = (!inView && !inViewR) || (farPoints && depth > thFar) || (P.skip && P.skip[i]);
    if (inView || inViewR) atomicAdd(O.count, 1);
}
__global__ __launch_bounds__(256) void k_frustum(FtDevFrame F, FtFrustumPose T, FtDevMapPoints P, float viewingCosLimit,
                                                 float logScaleFactor, int farPoints, float thFar, FtFrustumOut O) {
    frustum_point(F, T, P, viewingCosLimit, logScaleFactor, farPoints, thFar, O, blockIdx.x * 256 + threadIdx.x);
}
// isInFrustum for the local map points of every frame of a batch: blockIdx.y = frame (the counts are zeroed by the launcher)
__global__ __launch_bounds__(256) void k_frustum_batch(const FtBatchJob *__restrict__ jobs, Rebase rb, float viewingCosLimit,
                                                       float logScaleFactor, int farPoints, float thFar) {
    const FtBatchJob &J = jobs[blockIdx.y];
    FtDevMapPoints P = J.MP;
    P.skip = rb(P.skip); P.worldPos = rb(P.worldPos); P.normal = rb(P.normal); P.maxDist = rb(P.maxDist); P.minDist = rb(P.minDist);
    FtFrustumOut O = J.O;
    O.inView = rb(O.inView); O.inViewR = rb(O.inViewR); O.level = rb(O.level); O.levelR = rb(O.levelR);
    O.viewCos = rb(O.viewCos); O.viewCosR = rb(O.viewCosR); O.projX = rb(O.projX); O.projY = rb(O.projY);
    O.projXR = rb(O.projXR); O.projYR = rb(O.projYR); O.depth = rb(O.depth); O.depthR = rb(O.depthR);
    O.searchSkip = rb(O.searchSkip); O.count = rb(O.count);
    frustum_point(J.F, J.T, P, viewingCosLimit, logScaleFactor, farPoints, thFar, O, blockIdx.x * 256 + threadIdx.x);
}

// Result delivery of a search: up to three device blocks (dword granularity) written straight into pinned host memory by
// one kernel - pass results, raw outputs / frustum fields, and the pass flags - instead of one DMA copy each (a small copy
// is a few microseconds of work behind tens of microseconds of queueing).
struct FtBlocks {
    void *dst[3];
    const void *src[3];
    int words[3];
};
__global__ __launch_bounds__(256) void k_deliver_blocks(FtBlocks b) {
    const int t = blockIdx.x * 256 + threadIdx.x, T = gridDim.x * 256;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        unsigned *d = (unsigned *)b.dst[k];
        const unsigned *s = (const unsigned *)b.src[k];
        for (int i = t; i < b.words[k]; i += T) d[i] = s[i];
    }
}

__global__ __launch_bounds__(256) void k_fill_stride_u64(unsigned long long *p, int n, int strideWords, unsigned long long v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[(size_t)i * strideWords] = v;
}

// start of a claim iteration: list heads, flags and writer table = -1, the cache's meta words = ~0 ("not built") - one launch
__global__ __launch_bounds__(256) void k_fill_claims(int *p, int n, unsigned long long *meta, int nMeta, int strideWords) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = -1;
    if (i < nMeta) meta[(size_t)i * strideWords] = ~0ull;
}

__global__ __launch_bounds__(256) void k_fill_i32(int *p, int n, int v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// start of the claim iteration of every frame of a batch (blockIdx.y = frame): list heads and writer table = -1 (27 K words
// behind J.head: layoutBatch, tracked_batch.cpp), the frame's FT_BATCH_FLAGS flag words = -1, the cache's meta words = ~0, the frustum count = 0
__global__ __launch_bounds__(256) void k_fill_claims_batch(const FtBatchJob *__restrict__ jobs, Rebase rb) {
    const FtBatchJob &J = jobs[blockIdx.y];
    const int t = blockIdx.x * 256 + threadIdx.x, T = gridDim.x * 256;
    int *count = rb(J.O.count);
    if (t == 0 && count) *count = 0;
    int *replayed = rb(J.replayed);
    if (t == 0 && replayed) *replayed = -1;  // (k_replay_batch: this search's writes have not been replayed yet)
    int *err = rb(J.err);
    if (t == 0 && err) *err = 0;
    int *head = rb(J.head), *flags = rb(J.flags);
    if (t < FT_BATCH_FLAGS) flags[t] = -1;  // (also of a frame without points: "converged" is what the host reads there)
    if (J.nPoints <= 0) return;
    int *slow = rb(J.slow);
    if (t < 16) slow[t] = 0;
    unsigned long long *cache = rb(J.cache);
    const int words = 27 * J.K;
    for (int i = t; i < words; i += T) head[i] = -1;
    if (cache)
        for (int i = t; i < 2 * J.nPoints; i += T) cache[(size_t)i * (FT_CACHE_CAP + 1)] = ~0ull;
}

// Result delivery of a batch: record r (blockIdx.y) = one block of dwords written into pinned host memory; src[parity] lets a
// record follow the result buffer of the pass that ran last.
// The copy is bound by PCIe (a few hundred workgroups' stores in flight saturate it), so a record gets few workgroups that move
// 16 bytes per lane: the rest of the chip stays free for the kernels of the other batches in flight.
__global__ __launch_bounds__(256) void k_deliver_batch(const FtDeliverRec *__restrict__ recs, int parity) {
    const FtDeliverRec &R = recs[blockIdx.y];
    unsigned *d = (unsigned *)R.dst;
    const unsigned *s = (const unsigned *)R.src[parity];
    const int t = blockIdx.x * 256 + threadIdx.x, T = gridDim.x * 256;
    int done = 0;
    if ((((unsigned long long)(size_t)d | (unsigned long long)(size_t)s) & 15ull) == 0ull) {  // (uniform)
        const int quads = R.words >> 2;
        for (int i = t; i < quads; i += T) ((uint4 *)d)[i] = ((const uint4 *)s)[i];
        done = quads << 2;
    }
    for (int i = done + t; i < R.words; i += T) d[i] = s[i];
}

// The caller's point arrays, read in place out of pinned host memory, into the batch's arena: record r (blockIdx.y) = one array.
// 16 bytes per lane where source and destination allow it; the copy is PCIe-bound like the delivery, few workgroups per record.
__global__ __launch_bounds__(256) void k_gather_batch(const FtGatherRec *__restrict__ recs) {
    const FtGatherRec &R = recs[blockIdx.y];
    uint8_t *d = (uint8_t *)R.dst;
    const uint8_t *s = (const uint8_t *)R.src;
    const unsigned bytes = R.bytes;
    const unsigned t = blockIdx.x * 256 + threadIdx.x, T = gridDim.x * 256;
    unsigned done = 0;
    if ((((unsigned long long)(size_t)d | (unsigned long long)(size_t)s) & 15ull) == 0ull) {  // (uniform)
        const unsigned quads = bytes >> 4;
        for (unsigned i = t; i < quads; i += T) ((uint4 *)d)[i] = ((const uint4 *)s)[i];
        done = quads << 4;
    } else if ((((unsigned long long)(size_t)d | (unsigned long long)(size_t)s) & 3ull) == 0ull) {
        const unsigned words = bytes >> 2;
        for (unsigned i = t; i < words; i += T) ((unsigned *)d)[i] = ((const unsigned *)s)[i];
        done = words << 2;
    }
    for (unsigned i = done + t; i < bytes; i += T) d[i] = s[i];
}

}  // namespace

int ft_launch_gather_batch(hipStream_t st, const FtGatherRec *recs, int nRecs) {
    if (nRecs <= 0) return FT_OK;
    hipLaunchKernelGGL(k_gather_batch, dim3(2, nRecs), dim3(256), 0, st, recs);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_deliver_blocks(hipStream_t st, void *d0, const void *s0, size_t bytes0, void *d1, const void *s1, size_t bytes1,
                             void *d2, const void *s2, size_t bytes2) {
    FtBlocks b;
    b.dst[0] = d0; b.src[0] = s0; b.words[0] = (int)((bytes0 + 3) / 4);
    b.dst[1] = d1; b.src[1] = s1; b.words[1] = (int)((bytes1 + 3) / 4);
    b.dst[2] = d2; b.src[2] = s2; b.words[2] = (int)((bytes2 + 3) / 4);
    const int total = b.words[0] + b.words[1] + b.words[2];
    if (total <= 0) return FT_OK;
    hipLaunchKernelGGL(k_deliver_blocks, dim3(std::max(1, std::min(64, (total + 1023) / 1024))), dim3(256), 0, st, b);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_fill_stride_u64(hipStream_t st, unsigned long long *p, int n, int strideWords, unsigned long long v) {
    if (n <= 0) return FT_OK;
    hipLaunchKernelGGL(k_fill_stride_u64, dim3((n + 255) / 256), dim3(256), 0, st, p, n, strideWords, v);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_fill_claims(hipStream_t st, int *p, int n, unsigned long long *meta, int nMeta, int strideWords) {
    const int m = std::max(n, meta ? nMeta : 0);
    if (m <= 0) return FT_OK;
    hipLaunchKernelGGL(k_fill_claims, dim3((m + 255) / 256), dim3(256), 0, st, p, n, meta, meta ? nMeta : 0, strideWords);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_fill_i32(hipStream_t st, int *p, int n, int v) {
    if (n <= 0) return FT_OK;
    hipLaunchKernelGGL(k_fill_i32, dim3((n + 255) / 256), dim3(256), 0, st, p, n, v);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_frustum(hipStream_t st, const FtDevFrame &F, const FtFrustumPose &T, const FtDevMapPoints &P,
                      float viewingCosLimit, float logScaleFactor, int farPoints, float thFar, const FtFrustumOut &O) {
    int rc = ft_launch_fill_i32(st, O.count, 1, 0);
    if (rc != FT_OK) return rc;
    if (P.M <= 0) return FT_OK;
    hipLaunchKernelGGL(k_frustum, dim3((P.M + 255) / 256), dim3(256), 0, st, F, T, P, viewingCosLimit, logScaleFactor, farPoints,
                       thFar, O);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_build_grid(hipStream_t st, const FtDevFrame &F, int *gridStartL, int *gridStartR, float4 *recL, uint8_t *descL,
                         float4 *recR, uint8_t *descR) {
    hipLaunchKernelGGL(k_build_grid, dim3(F.nlevels, gridStartR ? 2 : 1), dim3(256), 0, st, F, gridStartL, gridStartR, recL, descL, recR,
                       descR);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

// ---- launches of a batch of frames (ft_tracked_batch, tracked_batch.cpp) ----
int ft_launch_build_grid_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxLevels, bool twoCam) {
    if (nFrames <= 0) return FT_OK;
    hipLaunchKernelGGL(k_build_grid_batch, dim3(maxLevels, twoCam ? 2 : 1, nFrames), dim3(256), 0, st, jobs, rebase_of(arena));
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_frustum_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxM, float viewingCosLimit, float logScaleFactor,
                            int farPoints, float thFar) {
    if (nFrames <= 0 || maxM <= 0) return FT_OK;
    hipLaunchKernelGGL(k_frustum_batch, dim3((maxM + 255) / 256, nFrames), dim3(256), 0, st, jobs, rebase_of(arena), viewingCosLimit,
                       logScaleFactor, farPoints, thFar);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_fill_claims_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxWords) {
    if (nFrames <= 0) return FT_OK;
    hipLaunchKernelGGL(k_fill_claims_batch, dim3(std::max(1, std::min(64, (maxWords + 1023) / 1024)), nFrames), dim3(256), 0, st, jobs,
                       rebase_of(arena));
    FT_HIP(hipGetLastError());
    return FT_OK;
}

#ifndef FT_DELIVER_BLOCKS
#define FT_DELIVER_BLOCKS 2  // workgroups per record
#endif
int ft_launch_deliver_batch(hipStream_t st, const FtDeliverRec *recs, int nRecs, int maxWords, int parity) {
    if (nRecs <= 0 || maxWords <= 0) return FT_OK;
    hipLaunchKernelGGL(k_deliver_batch, dim3(std::max(1, std::min(FT_DELIVER_BLOCKS, (maxWords + 1023) / 1024)), nRecs), dim3(256), 0, st, recs, parity);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

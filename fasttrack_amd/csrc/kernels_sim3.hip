// HIP kernels of the loop-closing projection matcher for gfx950 (wave64):
//   ORBmatcher::SearchByProjection(KeyFrame *pKF, Sim3f &Scw, vpPoints, vpMatched, th, ratioHamming)                       (reference src/ORBmatcher.cc:526-631)
//   ORBmatcher::SearchByProjection(KeyFrame *pKF, Sim3f &Scw, vpPoints, vpPointsKFs, vpMatched, vpMatchedKF, th, ratio)    (:633-745)
//
// The reference walks the points of a covisibility window in index order: the tests of the Sim3 Fuse overload in front of the
// window (depth, image, distance range, viewing angle, PredictScale), KeyFrame::GetFeaturesInArea without a level filter, and among
// the window's keypoints of octave level - 1 .. level whose vpMatched entry is NULL - held on entry or written by an earlier point
// of this call - the strict minimum of the descriptor distance, written when it is <= TH_LOW * ratioHamming.  The overloads differ
// in how the projection is rounded: mpCamera->project (:564) against the pinhole formula written out (:672-677).
// A point writes if and only if some free keypoint of its band is no farther than the threshold, and then it writes the smallest
// key (distance, cell x, cell y, index) among those: keys order by distance first.  So everything above the threshold is dropped
// before the sequential part, and a point without such a candidate never enters it:
//   k_sim3_grid        the per-octave grid of the keyframe's left camera (build_grid_body, search_dev.h), a workgroup per octave
//   k_sim3_candidates  a ROW of 16 lanes per (job, point), four points per wave: the front tests in the job's form, the window with
//                      the band as the scan's octave range (row_for_window), the keypoints free on entry with distance <= threshold
//                      as keys - the FT_SIM3_TOP smallest and their number - and the exit code of the point
//   k_sim3_resolve     a workgroup per job: the points that filed a key compacted in index order (the walk list); a taken bit per
//                      keypoint in LDS; wave 0 walks the list 64 points at a time, lane j holding point j's top record and which of
//                      its keys are still free, and gives each point its smallest free key - from the top record, or from a new
//                      scan of its window when all of that is taken and the window holds more.
// Three launches per call, whatever the jobs hold.  blockIdx.y is the job: what a workgroup reads of it sits at a uniform address.
#include <algorithm>

#include "search_dev.h"

namespace {

__global__ __launch_bounds__(256) void k_sim3_grid(const FtDevFrame F) {
    const FramePtrs Q = frame_ptrs(F, FT_NO_REBASE);
    build_grid_body(F, Q, blockIdx.x, 0, (int *)Q.gridStart[0], nullptr, (float4 *)Q.gridRec[0], (uint8_t *)Q.gridDesc[0], nullptr, nullptr);
}

// what the tests in front of the window leave of a point
struct Sim3Point {
    int stage;  // FT_FUSE_* (FT_FUSE_SEARCHED: the window is to be scanned)
    int level;
    float u, v, radius;
};

// :547-588 (:654-701) for point i of job J: the tests of fuse_point (kernels_fuse.hip) with the projection in the job's form
__device__ __forceinline__ Sim3Point sim3_point(const FtDevFrame &F, const FtSim3Job &J, const Rebase &rb, int i) {
    Sim3Point r;
    r.stage = FT_FUSE_SKIPPED;
    r.level = 0;
    r.u = r.v = r.radius = 0.f;
    const uint8_t *valid = rb(J.valid);
    if (valid && !valid[i]) return r;  // isBad() || spAlreadyFound.count(pMP)
    const float *wp = rb(J.P.worldPos) + 3 * (size_t)i;
    const float xw[3] = {wp[0], wp[1], wp[2]};
    float xc[3], uv[2];
    transform_pose(J.Tcw.m, J.Tcw.q, 1, xw, xc);
    r.stage = FT_FUSE_DEPTH;
    if (xc[2] < 0.0f) return r;  // (+-0 pass)
    if (J.handPinhole) {
        // :672-677: pKF->fx, fy, cx, cy whatever the camera model; no operation fuses with its neighbour
        const float invz = __fdiv_rn(1.0f, xc[2]);
        const float x = __fmul_rn(xc[0], invz), y = __fmul_rn(xc[1], invz);
        uv[0] = __fadd_rn(__fmul_rn(F.cam[0], x), F.cam[2]);
        uv[1] = __fadd_rn(__fmul_rn(F.cam[1], y), F.cam[3]);
    } else {
        project_cam(F, xc, uv);
    }
    r.stage = FT_FUSE_IMAGE;
    // KeyFrame::IsInImage (src/KeyFrame.cc:750-753): a NaN fails it
    if (!(uv[0] >= F.mnMinX && uv[0] < F.mnMaxX && uv[1] >= F.mnMinY && uv[1] < F.mnMaxY)) return r;
    const float PO[3] = {__fsub_rn(xw[0], J.Ow[0]), __fsub_rn(xw[1], J.Ow[1]), __fsub_rn(xw[2], J.Ow[2])};
    const float dist3D = norm3(PO);
    const float maxRaw = rb(J.P.maxDist)[i];
    const float maxDistance = __fmul_rn(1.2f, maxRaw), minDistance = __fmul_rn(0.8f, rb(J.P.minDist)[i]);
    r.stage = FT_FUSE_DISTANCE;
    if (dist3D < minDistance || dist3D > maxDistance) return r;
    const float *np = rb(J.P.normal) + 3 * (size_t)i;
    const float Pn[3] = {np[0], np[1], np[2]};
    r.stage = FT_FUSE_NORMAL;
    if ((double)dot3(PO, Pn) < 0.5 * (double)dist3D) return r;  // `PO.dot(Pn)<0.5*dist`: the float dot against a double product
    r.stage = FT_FUSE_SEARCHED;
    r.level = predict_scale(maxRaw, dist3D, J.logScaleFactor, F.nlevels);
    r.u = uv[0];
    r.v = uv[1];
    r.radius = __fmul_rn(J.th, F.sf[r.level]);  // `th*pKF->mvScaleFactors[nPredictedLevel]`: the int th converted to float
    return r;
}

#define FT_SIM3_PPB 16  // points per workgroup: 4 waves x 4 rows
__global__ __launch_bounds__(256) void k_sim3_candidates(const FtDevFrame F, const FtSim3Job *__restrict__ jobs, Rebase rb) {
    __shared__ unsigned rowLists[FT_SIM3_PPB][FT_ROW_LIST];
    unsigned *list = rowLists[threadIdx.x >> 4];
    const int lane = threadIdx.x & 63, sub = lane & 15, rowBase = lane & 48;
    const int i = (int)blockIdx.x * FT_SIM3_PPB + (int)(threadIdx.x >> 4);
    const FtSim3Job &J = jobs[blockIdx.y];
    if (i >= J.P.M) return;
    const FramePtrs Q = frame_ptrs(F, FT_NO_REBASE);
    const Sim3Point p = sim3_point(F, J, rb, i);
    int stage = p.stage, count = 0;
    unsigned long long t[FT_SIM3_TOP];
#pragma unroll
    for (int k = 0; k < FT_SIM3_TOP; k++) t[k] = KEY_NONE;
    if (stage == FT_FUSE_SEARCHED) {
        const Window w = cell_window(F, p.u, p.v, p.radius);
        bool any = false;
        if (!w.empty) {
            unsigned long long q[4];
            load_desc256(rb(J.P.desc), i, q);
            const int level = p.level, thr = J.thr;
            const int *matched = rb(J.matched);
            // the band [level - 1, level] (:608) is the scan's octave range: what reaches the visitor passed band and box
            row_for_window(F, Q, 0, w, level - 1, level, p.u, p.v, p.radius, sub, rowBase, list, [&](const WinEntry &kp, bool real) {
                any = any || real;
                const int dist = hamming256(q, kp.d);
                // `if(vpMatched[idx]) continue;` as far as the entry state decides it; `bestDist<=TH_LOW*ratioHamming` (:622)
                if (real && dist <= thr && matched[kp.idx] == -1) {
                    top_insert<FT_SIM3_TOP>(t, make_key(dist, kp.cx, kp.cy, kp.idx, kp.octave, false));
                    count++;
                }
            });
            any = ((unsigned)(__ballot(any) >> rowBase) & 0xffffu) != 0u;
            // `if(vIndices.empty())` (:592) looks at every octave: only the exit code depends on it when the band is empty
            if (!any && J.wantStage) {
                row_for_window(F, Q, 0, w, -1, -1, p.u, p.v, p.radius, sub, rowBase, list, [&](const WinEntry &, bool real) { any = any || real; });
                any = ((unsigned)(__ballot(any) >> rowBase) & 0xffffu) != 0u;
            }
        }
        stage = any ? FT_SIM3_NOWRITE : FT_FUSE_EMPTY;
        count = row_sum_i32(count);
    }
    // the FT_SIM3_TOP smallest keys of the row: the lanes' lists are ascending, so the row's minimum is some lane's head
    unsigned long long out = KEY_NONE;
#pragma unroll
    for (int k = 0; k < FT_SIM3_TOP; k++) {
        const unsigned long long m = row_min_u64(t[0]);
        if (sub == k) out = m;
        if (t[0] == m && m != KEY_NONE) {  // (keys are unique inside a window: one lane pops)
#pragma unroll
            for (int j = 0; j + 1 < FT_SIM3_TOP; j++) t[j] = t[j + 1];
            t[FT_SIM3_TOP - 1] = KEY_NONE;
        }
    }
    if (sub < FT_SIM3_TOP) rb(J.top)[(size_t)i * FT_SIM3_TOP + sub] = out;
    if (sub == 0) {
        FtSim3Proj pj;
        pj.u = p.u; pj.v = p.v; pj.radius = p.radius; pj.level = p.level;
        rb(J.proj)[i] = pj;
        rb(J.count)[i] = count;
        rb(J.pointKeypoint)[i] = -1;
        rb(J.stage)[i] = (uint8_t)stage;
    }
}

// LDS: taken[kp >> 5] bit kp & 31 = vpMatched[kp] was written by an earlier point of this call (the keypoints held on entry never
// became candidates).
#define FT_SIM3_RES_T 1024
__global__ __launch_bounds__(FT_SIM3_RES_T) void k_sim3_resolve(const FtDevFrame F, const FtSim3Job *__restrict__ jobs, Rebase rb) {
    extern __shared__ unsigned sim3_taken[];
    __shared__ int waveCnt[FT_SIM3_RES_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
    const FtSim3Job &J = jobs[blockIdx.y];
    const int M = J.P.M, nKeys = F.N;
    const int nWords = (nKeys + 31) / 32;
    unsigned *taken = sim3_taken;
    for (int k = tid; k < nWords; k += FT_SIM3_RES_T) taken[k] = 0u;
    const int *count = rb(J.count);
    int *walk = rb(J.walk);
    // the points that filed a key, in index order
    int nWalk = 0;  // (the same in every thread)
    for (int c0 = 0; c0 < M; c0 += FT_SIM3_RES_T) {
        const int i = c0 + tid;
        const bool has = i < M && count[i] > 0;
        const unsigned long long b = __ballot(has);
        if (lane == 0) waveCnt[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < FT_SIM3_RES_T / 64; w++) {
            const int c = waveCnt[w];
            total += c;
            before += w < wave ? c : 0;
        }
        if (has) walk[nWalk + before + __popcll(b & ((1ull << lane) - 1ull))] = i;
        nWalk += total;
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    if (tid >= 64) return;
    nWalk = __builtin_amdgcn_readfirstlane(nWalk);
    // the sequential walk, wave 0; every decision below is wave-uniform
    const FramePtrs Q = frame_ptrs(F, FT_NO_REBASE);
    const uint4 *top4 = (const uint4 *)rb(J.top);  // FT_SIM3_TOP keys = two 16-byte words per point
    const FtSim3Proj *proj = rb(J.proj);
    int *matched = rb(J.matched), *pointKeypoint = rb(J.pointKeypoint);
    uint8_t *stage = rb(J.stage);
    const int thr = J.thr;
    int nm = 0;
    uint4 nextA = make_uint4(~0u, ~0u, ~0u, ~0u), nextB = nextA;
    int nextCnt = 0, nextPt = 0;
    if (lane < nWalk) {
        nextPt = walk[lane];
        nextA = top4[2 * (size_t)nextPt];
        nextB = top4[2 * (size_t)nextPt + 1];
        nextCnt = count[nextPt];
    }
    for (int r0 = 0; r0 < nWalk; r0 += 64) {
        const uint4 curA = nextA, curB = nextB;
        const int curCnt = nextCnt, curPt = nextPt;
        if (r0 + 64 + lane < nWalk) {  // the next 64 points are on their way while these are decided
            nextPt = walk[r0 + 64 + lane];
            nextA = top4[2 * (size_t)nextPt];
            nextB = top4[2 * (size_t)nextPt + 1];
            nextCnt = count[nextPt];
        }
        const int nr = __builtin_amdgcn_readfirstlane(min(64, nWalk - r0));
        // Lane j holds point walk[r0 + j]: its top record, and which of those keys are still free (avail) - read from the taken bits
        // once per 64 points, then kept up to date in registers: every keypoint a point of this round takes is compared with the
        // record of every lane.  A decision is then one v_readlane of the lane's smallest free keypoint, where a look at the taken
        // bits for every key of every point cost an LDS round trip each (EXPERIMENTS.md section 20).
        const unsigned long long kq[FT_SIM3_TOP] = {((unsigned long long)curA.y << 32) | curA.x, ((unsigned long long)curA.w << 32) | curA.z,
                                                    ((unsigned long long)curB.y << 32) | curB.x, ((unsigned long long)curB.w << 32) | curB.z};
        int idx[FT_SIM3_TOP];
        unsigned avail = 0u;
#pragma unroll
        for (int q = 0; q < FT_SIM3_TOP; q++) {
            idx[q] = min(key_idx(kq[q]), nKeys - 1);
            const bool free_ = ((taken[idx[q] >> 5] >> (idx[q] & 31)) & 1u) == 0u;
            if (lane < nr && kq[q] != KEY_NONE && free_) avail |= 1u << q;
        }
        auto first_free = [&]() {  // (selects, last to first: no branch in the chain of decisions)
            int r = -1;
#pragma unroll
            for (int q = FT_SIM3_TOP - 1; q >= 0; q--) r = ((avail >> q) & 1u) ? idx[q] : r;
            return r;
        };
        int myBest = first_free();  // (ascending keys: the first free one is the smallest)
        int myMatch = -1;           // the keypoint this lane's point wrote
        for (int j = 0; j < nr; j++) {
            int bi = __builtin_amdgcn_readlane(myBest, j);
            if (bi < 0) {
                if (__builtin_amdgcn_readlane(curCnt, j) <= FT_SIM3_TOP) continue;  // every candidate of the point is taken
                // all of the top record is taken and the window holds more candidates: the window once more, against the taken bits
                // (with what this round has taken so far)
                if (myMatch >= 0) atomicOr(&taken[myMatch >> 5], 1u << (myMatch & 31));
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int pt = __builtin_amdgcn_readlane(curPt, j);
                const FtSim3Proj pj = proj[pt];
                const Window w = cell_window(F, pj.u, pj.v, pj.radius);
                const unsigned long long *dp = (const unsigned long long *)(rb(J.P.desc) + (size_t)pt * 32);
                const unsigned long long d1[4] = {dp[0], dp[1], dp[2], dp[3]};
                unsigned long long k0 = KEY_NONE;
                for_window(F, Q, 0, Q.keys, nKeys, w, pj.level - 1, pj.level, lane, [&](const WinEntry &kp) {
                    if (!in_box(kp, pj.u, pj.v, pj.radius, pj.level - 1, pj.level)) return;
                    const int i2 = min(kp.idx, nKeys - 1);
                    if (matched[i2] != -1 || ((taken[i2 >> 5] >> (i2 & 31)) & 1u)) return;  // held on entry, or written since
                    const int dist = hamming256(d1, kp.d);
                    if (dist > thr) return;
                    const unsigned long long key = make_key(dist, kp.cx, kp.cy, kp.idx, kp.octave, false);
                    k0 = key < k0 ? key : k0;
                });
                const unsigned long long best = wave_min_u64(k0);
                if (best == KEY_NONE) continue;
                bi = min(key_idx(best), nKeys - 1);
            }
            // every candidate is within the threshold: the point writes (:622-626)
            if (lane == j) myMatch = bi;
            nm++;
#pragma unroll
            for (int q = 0; q < FT_SIM3_TOP; q++)
                if (idx[q] == bi) avail &= ~(1u << q);
            myBest = first_free();
        }
        // the taken bits of the round in one LDS instruction, where a read-modify-write per decision put an LDS round trip into
        // every step of the chain
        if (myMatch >= 0) atomicOr(&taken[myMatch >> 5], 1u << (myMatch & 31));
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the next round reads the taken bits
        __builtin_amdgcn_wave_barrier();
        if (lane < nr && myMatch >= 0) {
            pointKeypoint[curPt] = myMatch;
            matched[myMatch] = curPt;
            stage[curPt] = (uint8_t)FT_FUSE_SEARCHED;
        }
    }
    if (lane == 0) *rb(J.nMatches) = nm;
}

}  // namespace

int ft_launch_sim3_grid(hipStream_t st, const FtDevFrame &F) {
    hipLaunchKernelGGL(k_sim3_grid, dim3(F.nlevels), dim3(256), 0, st, F);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_sim3_candidates(hipStream_t st, const FtDevFrame &F, void *arena, const FtSim3Job *jobs, int nJobs, int maxM) {
    hipLaunchKernelGGL(k_sim3_candidates, dim3((maxM + FT_SIM3_PPB - 1) / FT_SIM3_PPB, nJobs), dim3(256), 0, st, F, jobs, rebase_of(arena));
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_sim3_resolve(hipStream_t st, const FtDevFrame &F, void *arena, const FtSim3Job *jobs, int nJobs) {
    const size_t lds = ft_sim3_lds_bytes(F.N);
    if (lds > FT_INIT_MAX_LDS) {
        ft_set_error("SearchByProjection(KeyFrame, Sim3): the keyframe's keypoints exceed the taken bits of the resolution");
        return FT_ERR_CAPACITY;
    }
    const int rc = ft_allow_max_lds<k_sim3_resolve>();
    if (rc != FT_OK) return rc;
    hipLaunchKernelGGL(k_sim3_resolve, dim3(1, nJobs), dim3(FT_SIM3_RES_T), lds, st, F, jobs, rebase_of(arena));
    FT_HIP(hipGetLastError());
    return FT_OK;
}

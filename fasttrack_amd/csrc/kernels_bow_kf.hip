// HIP kernels of ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vpMatches12) (reference src/ORBmatcher.cc:864-1004)
// for gfx950 (wave64): keyframe 1 against every neighbour of a call (LoopClosing::DetectCommonRegionsFromBoW,
// src/LoopClosing.cc:657-668), two launches whatever the number of neighbours.
//   k_bow_kf_match   blockIdx.y = neighbour.  The unit of work is one (node of keyframe 1, neighbour) pair, a WAVE per unit:
//                    binary search for the node on the neighbour's side (the reference's lower_bound walk visits exactly the
//                    common keys, :892-981), then k_search_by_bow's walk turned around - the node's keyframe-2 candidates stay
//                    resident across the lanes (lane l holds the list positions l, l + 64, ...: index, descriptor, and a "free"
//                    bit that is set for a candidate that has a good map point and passes the mvKeysUn test, :919-929), the
//                    node's keyframe-1 features are taken one after another in list order (:896; each sees the claims of the
//                    ones in front of it), 64 of them loaded at a time and the current one broadcast by v_readlane.  The wave's
//                    two smallest (distance << 20 | list position) keys are bestDist1 / bestIdx2 and bestDist2: strict < in
//                    scan order (:935-944) = the first of the list with the smallest distance.  Acceptance (:947-949) clears the
//                    free bit in the lane that holds the candidate (vbMatched2, :952) and that lane writes matches12[idx1].
//                    vbMatched2 is only ever read for features of the node that wrote it (a feature sits in one FeatureVector
//                    entry), so the units are independent.
//                    A list of more than 256 entries does not fit the registers: its claims go through job->claimed[], written
//                    and read back by the SAME lane (position & 63) as in k_search_by_bow's tail, so no ordering between lanes is
//                    needed and no list length is an error.
//   k_bow_kf_finish  a workgroup per neighbour: rotation histogram over the matches (:954-964), ComputeThreeMaxima, the removal
//                    (:983-1001), nmatches.
// Why a wave and not a row of 16 lanes per unit.  Node sizes, from the restatement's stats (tests/bow_kf_ref.py): on the bench
// shape (tests/tools/bench_bow_kf.py: 2 000 features, half of them with a point, k = 10, L = 5, levelsup 3; 600 units = 100 shared
// nodes x 6 neighbours) keyframe 2's lists hold 19 entries at the median, 27 at the 90th percentile, 41 at most, of which 9 / 15 /
// 23 are eligible (95 % of the units have <= 16 eligible candidates, all <= 64); keyframe 1's lists 19.5 / 25 / 29 with 10 / 13 /
// 21 eligible.  The ~100-node scenarios of tests/bow_kf_cases.py (500 - 700 features) have lists of 4 - 6 at the median, 18 at most.
// A row would fill its lanes better, but the lanes are not what a call waits for: 100 nodes x 36 neighbours are 3 600 units for the
// 1 024 SIMDs of the device, each of which holds several waves, so every unit is resident from the start either way and the
// kernel's time is the longest sequential chain of keyframe-1 features in one unit.  A step of that chain is no longer in a wave:
// the unit's control flow is wave-uniform, so the current feature is broadcast through scalar registers (v_readlane; a row
// would need ds_bpermute through the LDS crossbar or a load per step), the whole list (not only its eligible part: no
// compaction step) fits the registers up to 256 entries instead of 64, and the memory path is k_search_by_bow's proven one.
// A row variant was not built, so its time is not measured; EXPERIMENTS.md has the measured times of this one.
#include <algorithm>

#include "ft_internal.h"
#include "ft_search.h"
#include "rot_filter_dev.h"
#include "wave_ops.h"

namespace {

#define FT_BOWKF_R 4  // candidates per lane held in registers: lists of up to 64 * FT_BOWKF_R entries
#define FT_BOWKF_FIN_T 256

// !(NLeft != -1 && idx >= mvKeysUn.size()) && pMP && !pMP->isBad()  (:899-907 for keyframe 1, :919-929 for keyframe 2)
__device__ __forceinline__ bool eligible(int nLeft, int nUn, const uint8_t *has, unsigned idx) {
    if (nLeft != -1 && (int)idx >= nUn) return false;
    return has[idx] != 0;
}

__global__ __launch_bounds__(256) void k_bow_kf_match(FtBowKfCall T) {
    uint8_t *arena = T.arena;
    const int lane = threadIdx.x & 63;
    const int a = (int)blockIdx.x * 4 + wave_index();
    const FtBowArenaSide &K1 = T.K1;
    if (a >= K1.fv.nNodes) return;
    const FtBowKfJob *job = at<FtBowKfJob>(arena, T.jobs) + blockIdx.y;
    const FtBowArenaSide K2 = job->K2;
    if (K2.fv.n <= 0 || K2.fv.nNodes <= 0) return;  // nothing of an empty neighbour is dereferenced
    const int lo = fv_find_node(at<unsigned>(arena, K2.fv.nodes), K2.fv.nNodes, at<unsigned>(arena, K1.fv.nodes)[a]);
    if (lo < 0) return;
    const int fBeg = at<int>(arena, K2.fv.offsets)[lo], fCnt = at<int>(arena, K2.fv.offsets)[lo + 1] - fBeg;
    const int kBeg = at<int>(arena, K1.fv.offsets)[a], kCnt = at<int>(arena, K1.fv.offsets)[a + 1] - kBeg;
    if (fCnt <= 0 || kCnt <= 0) return;
    const unsigned *feats1 = at<unsigned>(arena, K1.fv.feats) + kBeg, *feats2 = at<unsigned>(arena, K2.fv.feats) + fBeg;
    const uint8_t *has1 = at<uint8_t>(arena, K1.hasPoint), *has2 = at<uint8_t>(arena, K2.hasPoint);
    const uint8_t *desc1 = at<uint8_t>(arena, K1.desc), *desc2 = at<uint8_t>(arena, K2.desc);
    int *matches = (int *)(arena + job->matches);
    // a unit without an eligible feature on either side is done before it touches a descriptor
    {
        bool any1 = false, any2 = false;
        for (int p = lane; p < kCnt; p += 64) any1 |= eligible(K1.nLeft, K1.nUn, has1, feats1[p]);
        for (int p = lane; p < fCnt; p += 64) any2 |= eligible(K2.nLeft, K2.nUn, has2, feats2[p]);
        if (!__ballot(any1) || !__ballot(any2)) return;
    }
    constexpr unsigned NONE = (256u << 20) | 0xfffffu;  // bestDist = 256, no position
    // bestDist1 < TH_LOW, strictly (:947; not the <= of the KeyFrame, Frame overload at :426), and the ratio as one fp32 product
    auto accepted = [&](unsigned k0, unsigned k1) {
        const int bestDist1 = (int)(k0 >> 20), bestDist2 = (int)(k1 >> 20);
        return bestDist1 < FT_TH_LOW && (float)bestDist1 < __fmul_rn(T.nnRatio, (float)bestDist2);
    };
    constexpr int R = FT_BOWKF_R;
    if (fCnt <= 64 * R) {
        unsigned fIdx[R];
        unsigned long long f0[R], f1[R], f2[R], f3[R];
        unsigned freeMask = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            fIdx[r] = 0u;
            f0[r] = f1[r] = f2[r] = f3[r] = 0ull;
            if (r * 64 < fCnt) {  // (wave-uniform)
                const int p = r * 64 + lane;
                fIdx[r] = feats2[min(p, fCnt - 1)];  // idle lanes read the last entry of the list
                const unsigned long long *q = (const unsigned long long *)(desc2 + (size_t)fIdx[r] * 32);
                f0[r] = q[0]; f1[r] = q[1]; f2[r] = q[2]; f3[r] = q[3];
                freeMask |= ((p < fCnt && eligible(K2.nLeft, K2.nUn, has2, fIdx[r])) ? 1u : 0u) << r;
            }
        }
        for (int k0i = 0; k0i < kCnt; k0i += 64) {
            const int cnt = min(64, kCnt - k0i);
            const unsigned kIdx = feats1[k0i + min(lane, cnt - 1)];
            const int el = (lane < cnt && eligible(K1.nLeft, K1.nUn, has1, kIdx)) ? 1 : 0;
            const unsigned long long *qk = (const unsigned long long *)(desc1 + (size_t)kIdx * 32);
            const unsigned long long d0 = qk[0], d1 = qk[1], d2 = qk[2], d3 = qk[3];
            for (int jj = 0; jj < cnt; jj++) {
                const int j = __builtin_amdgcn_readfirstlane(jj);
                if (!__builtin_amdgcn_readlane(el, j)) continue;
                const int idx1 = __builtin_amdgcn_readlane((int)kIdx, j);
                const unsigned long long b0 = wave_readlane_u64(d0, j), b1 = wave_readlane_u64(d1, j), b2 = wave_readlane_u64(d2, j), b3 = wave_readlane_u64(d3, j);
                unsigned l0 = NONE, l1 = NONE;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const unsigned dist = (unsigned)(__popcll(b0 ^ f0[r]) + __popcll(b1 ^ f1[r]) + __popcll(b2 ^ f2[r]) + __popcll(b3 ^ f3[r]));
                    const unsigned key = (freeMask >> r & 1u) ? ((dist << 20) | (unsigned)(r * 64 + lane)) : NONE;
                    const unsigned larger = max(key, l0);
                    l0 = min(l0, key);
                    l1 = min(l1, larger);
                }
                wave_two_min(l0, l1);
                if (!accepted(l0, l1)) continue;
                const int p = (int)(l0 & 0xfffffu);
                if ((p & 63) == lane) {
#pragma unroll
                    for (int r = 0; r < R; r++)
                        if ((p >> 6) == r) {
                            freeMask &= ~(1u << r);         // vbMatched2[bestIdx2] = true (:952)
                            matches[idx1] = (int)fIdx[r];  // vpMatches12[idx1] = vpMapPoints2[bestIdx2] (:951)
                        }
                }
            }
        }
        return;
    }
    int *claimed = (int *)(arena + job->claimed);
    for (int ik = 0; ik < kCnt; ik++) {
        const unsigned idx1 = feats1[ik];
        if (!eligible(K1.nLeft, K1.nUn, has1, idx1)) continue;
        const unsigned long long *dk = (const unsigned long long *)(desc1 + (size_t)idx1 * 32);
        const unsigned long long k0 = dk[0], k1 = dk[1], k2 = dk[2], k3 = dk[3];
        unsigned l0 = NONE, l1 = NONE;
        for (int p = lane; p < fCnt; p += 64) {
            const unsigned idx2 = feats2[p];
            if (!eligible(K2.nLeft, K2.nUn, has2, idx2)) continue;
            if (__hip_atomic_load(claimed + idx2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) continue;  // vbMatched2 (:925)
            const unsigned long long *q = (const unsigned long long *)(desc2 + (size_t)idx2 * 32);
            const unsigned dist = (unsigned)(__popcll(k0 ^ q[0]) + __popcll(k1 ^ q[1]) + __popcll(k2 ^ q[2]) + __popcll(k3 ^ q[3]));
            const unsigned key = (dist << 20) | (unsigned)p;
            const unsigned larger = max(key, l0);
            l0 = min(l0, key);
            l1 = min(l1, larger);
        }
        wave_two_min(l0, l1);
        if (!accepted(l0, l1)) continue;
        const int p = (int)(l0 & 0xfffffu);
        if ((p & 63) == lane) {
            const unsigned idx2 = feats2[p];
            __hip_atomic_store(claimed + idx2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            matches[idx1] = (int)idx2;
        }
    }
}

__global__ __launch_bounds__(FT_BOWKF_FIN_T) void k_bow_kf_finish(FtBowKfCall T) {
    uint8_t *arena = T.arena;
    const FtBowKfJob *job = at<FtBowKfJob>(arena, T.jobs) + blockIdx.x;
    const float *angle1 = at<float>(arena, T.K1.angles), *angle2 = at<float>(arena, job->K2.angles);
    // vKeysUn1[idx1].angle - vKeysUn2[bestIdx2].angle (:956); the removal :983-1001
    rot_filter_rows<FT_BOWKF_FIN_T>((int *)(arena + job->matches), T.K1.fv.n, T.checkOrientation, (int *)(arena + T.nMatches) + blockIdx.x,
                                    [&](int i, int m) { return init_bin(angle1[i], angle2[m]); });
}

}  // namespace

int ft_launch_bow_kf_match(hipStream_t st, const FtBowKfCall &T) {
    const dim3 grid((unsigned)std::max((T.K1.fv.nNodes + 3) / 4, 1), (unsigned)T.nNeighbours);
    hipLaunchKernelGGL(k_bow_kf_match, grid, dim3(256), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_bow_kf_finish(hipStream_t st, const FtBowKfCall &T) {
    hipLaunchKernelGGL(k_bow_kf_finish, dim3((unsigned)T.nNeighbours), dim3(FT_BOWKF_FIN_T), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

// HIP kernels of MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:329-403) for gfx950 (wave64): every map point of
// a call, at most three launches whatever the number of points - one per class of list length N that occurs in the call.
//   k_distinct_short  N <= 16.  Typical tracks hold 2 - 8 observations, so a wave serves several points: a SUB-GROUP of 8 lanes
//                     (N <= 8; 8 points per wave) or of 16 lanes (9 <= N <= 16; 4 per wave).  The workgroups of the 8-lane lists
//                     come first in the grid, those of the 16-lane lists behind them.  Lane i of a sub-group keeps descriptor i
//                     in eight VGPRs and puts it into the LDS; descriptor j comes back as two 16-byte reads that are a broadcast
//                     inside the sub-group (4 or 8 distinct addresses per wave); the lane's row d(i, 0 .. G - 1) stays in
//                     registers (the loops over j are unrolled).
//   k_distinct_wave   N <= 64.  A wave per point, lane i = descriptor i.  Descriptor j is broadcast through v_readlane (j is
//                     wave-uniform); the row goes to the LDS as 16-bit values, j-major (lane i writes and later reads
//                     row[j * 64 + i] - consecutive lanes hit consecutive halfwords, and no lane reads what another one wrote,
//                     so the wave needs no barrier).
//   k_distinct_block  N <= FT_DISTINCT_MAX_OBSERVATIONS.  A workgroup of 1 024 threads per point, the descriptors staged in the
//                     LDS (32 B x N).  A row i of the matrix belongs to the 16 lanes of a DPP row: lane s of them takes
//                     j = s, s + 16, ..., and the 16 counts of a search step are summed by DPP, so the lanes of a row agree on
//                     every step without a barrier.  The workgroup takes 64 rows at a time.  A row is not stored: each step of
//                     the median search recomputes d(i, j) from the LDS.  (With a thread per row a list of 80 kept two waves
//                     busy for 9 x 80 distances each: 38 us for three such points; EXPERIMENTS.md.)
// The median (:388-390) is an order statistic, so nothing is sorted: with k = (N - 1) / 2 = (size_t)(0.5 * (N - 1)), the element
// at index k of the ascending row is the smallest v with #{j : d(i, j) <= v} >= k + 1 - found by bisection over v in [0, 256]
// (nine steps; 256 always satisfies the condition).  A distance is an int everywhere except in k_distinct_wave's LDS row, where it
// is 16 bits wide: 256 fits.
// BestIdx (:384-397: BestMedian = INT_MAX, strict <, i ascending = the FIRST row with the smallest median) is the minimum of the
// keys median << 20 | i over the rows (i < 2^10, median <= 256), taken by DPP steps inside the sub-group, over the wave, or over
// the workgroup's waves.  Every result is written with plain vector stores; points with an empty list have no job, so nothing
// of theirs is written.
#include <algorithm>

#include "ft_internal.h"
#include "ft_search.h"
#include "wave_ops.h"

namespace {

#define FT_DISTINCT_T 256
#define FT_DISTINCT_BLOCK_T 1024  // k_distinct_block: 64 rows of 16 lanes
#define FT_DISTINCT_NOKEY 0xffffffffu

__device__ __forceinline__ int hamming_u4(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
           __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// minimum over the sub-group of G lanes (8: quad steps and row_half_mirror, all inside an aligned group of 8; 16: the row), in
// every lane of it.  Called with all 64 lanes active.
template <int G>
__device__ __forceinline__ unsigned group_min_u32(unsigned v) {
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true));  // row_half_mirror
    if (G == 16) v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true));  // row_mirror
    return v;
}

// the part of k_distinct_short that serves `nJobs` points in sub-groups of G lanes; `wg` counts the workgroups of this part.
// No thread leaves before the barrier and the DPP steps.
template <int G>
__device__ __forceinline__ void distinct_short(const FtDistinctCall &T, const int *jobs, int nJobs, int wg, uint4 *sd) {
    uint8_t *arena = T.arena;
    const int tid = threadIdx.x, grp = tid / G, i = tid % G;
    const int slot = wg * (FT_DISTINCT_T / G) + grp;
    const bool live = slot < nJobs;
    int p = 0, beg = 0, N = 0;
    if (live) {
        p = jobs[slot];
        const int *offsets = at<int>(arena, T.offsets);
        beg = offsets[p];
        N = min(offsets[p + 1] - beg, G);  // (the host files a point here only when its list fits)
    }
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (i < N) {
        const uint4 *q = (const uint4 *)(arena + T.desc + ((size_t)beg + i) * 32);
        a0 = q[0];
        a1 = q[1];
    }
    sd[2 * tid] = a0;
    sd[2 * tid + 1] = a1;
    __syncthreads();
    int d[G];
#pragma unroll
    for (int j = 0; j < G; j++) {
        // every slot of the sub-group is read, so that the G reads are in flight together; beyond the list (the slot holds
        // zeros) the distance becomes >= 0x7fff: never counted
        const uint4 b0 = sd[2 * (grp * G + j)], b1 = sd[2 * (grp * G + j) + 1];
        d[j] = hamming_u4(a0, a1, b0, b1) | (j < N ? 0 : 0x7fff);
    }
    const int need = ((N - 1) >> 1) + 1;
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < G; j++) cnt += d[j] <= mid ? 1 : 0;
        if (cnt >= need) hi = mid;
        else lo = mid + 1;
    }
    const unsigned key = i < N ? ((unsigned)lo << 20) | (unsigned)i : FT_DISTINCT_NOKEY;
    const unsigned best = group_min_u32<G>(key);
    if (i < N && key == best) {  // the lane that holds vDescriptors[BestIdx]
        ((int *)(arena + T.bestIdx))[p] = i;
        ((int *)(arena + T.bestMedian))[p] = lo;
        uint4 *o = (uint4 *)(arena + T.outDesc + (size_t)p * 32);
        o[0] = a0;
        o[1] = a1;
    }
}

__global__ __launch_bounds__(FT_DISTINCT_T) void k_distinct_short(FtDistinctCall T) {
    __shared__ uint4 sd[2 * FT_DISTINCT_T];
    const int *jobs = at<int>(T.arena, T.jobs);
    const int wg8 = (T.n8 + FT_DISTINCT_T / 8 - 1) / (FT_DISTINCT_T / 8);
    if ((int)blockIdx.x < wg8) distinct_short<8>(T, jobs, T.n8, (int)blockIdx.x, sd);
    else distinct_short<16>(T, jobs + T.n8, T.n16, (int)blockIdx.x - wg8, sd);
}

__global__ __launch_bounds__(FT_DISTINCT_T) void k_distinct_wave(FtDistinctCall T) {
    __shared__ unsigned short rows[FT_DISTINCT_T / 64][64 * 64];
    uint8_t *arena = T.arena;
    const int lane = threadIdx.x & 63, w = wave_index();
    const int slot = (int)blockIdx.x * (FT_DISTINCT_T / 64) + w;
    if (slot >= T.nWave) return;  // (wave-uniform; the kernel has no barrier)
    const int p = __builtin_amdgcn_readfirstlane(at<int>(arena, T.jobs)[T.n8 + T.n16 + slot]);
    const int *offsets = at<int>(arena, T.offsets);
    const int beg = __builtin_amdgcn_readfirstlane(offsets[p]);
    const int N = min(__builtin_amdgcn_readfirstlane(offsets[p + 1]) - beg, 64);
    unsigned a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (lane < N) {
        const uint4 *q = (const uint4 *)(arena + T.desc + ((size_t)beg + lane) * 32);
        const uint4 x = q[0], y = q[1];
        a[0] = x.x; a[1] = x.y; a[2] = x.z; a[3] = x.w;
        a[4] = y.x; a[5] = y.y; a[6] = y.z; a[7] = y.w;
    }
    unsigned short *row = rows[w];
    for (int j = 0; j < N; j++) {
        int dist = 0;
#pragma unroll
        for (int r = 0; r < 8; r++) dist += __popc(a[r] ^ (unsigned)__builtin_amdgcn_readlane((int)a[r], j));
        row[j * 64 + lane] = (unsigned short)dist;  // <= 256
    }
    const int need = ((N - 1) >> 1) + 1;
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
#pragma unroll 8
        for (int j = 0; j < N; j++) cnt += (int)row[j * 64 + lane] <= mid ? 1 : 0;  // (unrolled: the reads are in flight together)
        if (cnt >= need) hi = mid;
        else lo = mid + 1;
    }
    const unsigned key = lane < N ? ((unsigned)lo << 20) | (unsigned)lane : FT_DISTINCT_NOKEY;
    const unsigned best = wave_min_u32(key);
    if (lane < N && key == best) {
        ((int *)(arena + T.bestIdx))[p] = lane;
        ((int *)(arena + T.bestMedian))[p] = lo;
        uint4 *o = (uint4 *)(arena + T.outDesc + (size_t)p * 32);
        o[0] = make_uint4(a[0], a[1], a[2], a[3]);
        o[1] = make_uint4(a[4], a[5], a[6], a[7]);
    }
}

__global__ __launch_bounds__(FT_DISTINCT_BLOCK_T) void k_distinct_block(FtDistinctCall T) {
    __shared__ uint4 sd[2 * FT_DISTINCT_MAX_OBSERVATIONS];
    __shared__ unsigned waveBest[FT_DISTINCT_BLOCK_T / 64];
    uint8_t *arena = T.arena;
    const int tid = threadIdx.x, sub = tid & 15, rowSlot = tid >> 4;
    const int p = at<int>(arena, T.jobs)[T.n8 + T.n16 + T.nWave + (int)blockIdx.x];
    const int *offsets = at<int>(arena, T.offsets);
    const int beg = offsets[p];
    const int N = min(offsets[p + 1] - beg, FT_DISTINCT_MAX_OBSERVATIONS);  // (the host rejects a longer list)
    const uint4 *src = (const uint4 *)(arena + T.desc + (size_t)beg * 32);
    for (int r = tid; r < 2 * N; r += FT_DISTINCT_BLOCK_T) sd[r] = src[r];
    __syncthreads();
    const int need = ((N - 1) >> 1) + 1;
    unsigned key = FT_DISTINCT_NOKEY;
    for (int base = 0; base < N; base += FT_DISTINCT_BLOCK_T / 16) {  // (uniform over the workgroup)
        const int i = base + rowSlot;
        const int ii = min(i, N - 1);  // the DPP row of a slot beyond the list recomputes the last row; its key is dropped
        const uint4 a0 = sd[2 * ii], a1 = sd[2 * ii + 1];
        int lo = 0, hi = 256;
        while (lo < hi) {  // the 16 lanes of a DPP row hold the same lo / hi: they stay together, row_sum_i32 sees all of them
            const int mid = (lo + hi) >> 1;
            int cnt = 0;
#pragma unroll 4
            for (int j = sub; j < N; j += 16) cnt += hamming_u4(a0, a1, sd[2 * j], sd[2 * j + 1]) <= mid ? 1 : 0;  // (as above)
            cnt = row_sum_i32(cnt);
            if (cnt >= need) hi = mid;
            else lo = mid + 1;
        }
        if (i < N) key = min(key, ((unsigned)lo << 20) | (unsigned)i);
    }
    const unsigned m = wave_min_u32(key);
    if ((tid & 63) == 0) waveBest[tid >> 6] = m;
    __syncthreads();
    unsigned best = waveBest[0];
#pragma unroll
    for (int w = 1; w < FT_DISTINCT_BLOCK_T / 64; w++) best = min(best, waveBest[w]);
    const int bestIdx = (int)(best & 0xfffffu);
    if (tid == 0) {
        ((int *)(arena + T.bestIdx))[p] = bestIdx;
        ((int *)(arena + T.bestMedian))[p] = (int)(best >> 20);
    }
    if (tid < 2) ((uint4 *)(arena + T.outDesc + (size_t)p * 32))[tid] = sd[2 * bestIdx + tid];
}

}  // namespace

int ft_launch_distinct_short(hipStream_t st, const FtDistinctCall &T) {
    const int wg = (T.n8 + FT_DISTINCT_T / 8 - 1) / (FT_DISTINCT_T / 8) + (T.n16 + FT_DISTINCT_T / 16 - 1) / (FT_DISTINCT_T / 16);
    hipLaunchKernelGGL(k_distinct_short, dim3((unsigned)wg), dim3(FT_DISTINCT_T), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_distinct_wave(hipStream_t st, const FtDistinctCall &T) {
    const int wg = (T.nWave + FT_DISTINCT_T / 64 - 1) / (FT_DISTINCT_T / 64);
    hipLaunchKernelGGL(k_distinct_wave, dim3((unsigned)wg), dim3(FT_DISTINCT_T), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_distinct_block(hipStream_t st, const FtDistinctCall &T) {
    hipLaunchKernelGGL(k_distinct_block, dim3((unsigned)T.nBlock), dim3(FT_DISTINCT_BLOCK_T), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

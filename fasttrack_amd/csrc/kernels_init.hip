// HIP kernels of the monocular initialisation matcher for gfx950 (wave64):
//   ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)   (reference src/ORBmatcher.cc:747-862)
//
// The reference walks the level-0 keypoints of F1 in index order; a keypoint takes the best candidate of its window in F2
// unless that candidate is held at a distance that is not larger (vMatchedDistance[i2] <= dist: skipped), and a strictly
// closer keypoint takes a match AWAY from its owner, who stays unmatched.  The distances do not depend on that state, the
// decisions do, so the work is split (the terms ROW, ORD and the candidate word: ft_search.h):
//   k_init_prepare     the rows of F1 (a block scan over the octaves) and the ords of F2's level-0 grid entries
//   k_init_candidates  a wave per row: the window's candidates (distance, ord) into the row's segment, and the
//                      FT_INIT_TOP smallest of them, ascending, into the row's top record
//   k_init_resolve     one workgroup: the sequential part.  vMatchedDistance / vnMatches21 live in LDS, one word per ord;
//                      wave 0 walks the rows in order.  The smallest candidate that is not skipped is the reference's best
//                      (ascending words = ascending distance, then the order of GetFeaturesInArea), the next one that is
//                      not skipped its second best, so a row is decided from its top record unless more than
//                      FT_INIT_TOP - 2 of those are skipped - only then the wave reads the segment.  Then, by the whole
//                      workgroup: rotation histogram (an evicted row stays in its bin, :824), ComputeThreeMaxima, the
//                      removal, nmatches, vnMatches12 and vbPrevMatched.
// Three launches per call, whatever the frames hold.
#include <algorithm>
#include <climits>

#include "ft_search.h"
#include "rot_filter_dev.h"
#include "wave_ops.h"

namespace {

#define FT_INIT_ORD_MASK ((1u << FT_INIT_ORD_BITS) - 1u)
#define FT_INIT_PREP_T 1024
#define FT_INIT_TH_LOW 50  // ORBmatcher::TH_LOW (src/ORBmatcher.cc:42)

__device__ __forceinline__ int init_cell_of(const FtDevFrame &F, float x, float y) {  // Frame::PosInGrid, as k_build_grid files a keypoint
    const int cx = (int)roundf(__fmul_rn(__fsub_rn(x, F.mnMinX), F.invW));
    const int cy = (int)roundf(__fmul_rn(__fsub_rn(y, F.mnMinY), F.invH));
    if (cx < 0 || cx >= FT_GRID_COLS || cy < 0 || cy >= FT_GRID_ROWS) return -1;
    return cx * FT_GRID_ROWS + cy;
}

// block 0: rows[] = the keypoints of F1 with octave 0, ascending (octave > 0 is skipped at :764; the host admits no negative octave).
// blocks 1 ..: the ord of every entry of octave 0 of F2's grid: the entries of a cell are filed in no particular order
// (k_build_grid), the reference visits them by ascending index - the ord of an entry is its cell's first position plus
// the number of entries of the cell with a smaller index.
__global__ __launch_bounds__(FT_INIT_PREP_T) void k_init_prepare(FtInitSearch S) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int *gs = S.F2.gridStart[0];  // octave 0
    if (blockIdx.x == 0) {
        __shared__ int wsum[FT_INIT_PREP_T / 64];
        const int per = (S.N1 + FT_INIT_PREP_T - 1) / FT_INIT_PREP_T;
        const int i0 = min(tid * per, S.N1), i1 = min(i0 + per, S.N1);
        int mine = 0;
        for (int i = i0; i < i1; i++) mine += S.keys1[i].octave == 0 ? 1 : 0;
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(incl, d);
            if (lane >= d) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int r = incl - mine, total = 0;
        for (int w = 0; w < FT_INIT_PREP_T / 64; w++) {
            if (w < wave) r += wsum[w];
            total += wsum[w];
        }
        for (int i = i0; i < i1; i++)
            if (S.keys1[i].octave == 0) {
                if (r < S.cap1) S.rows[r] = i;
                r++;
            }
        if (tid == 0) {
            const int n2 = gs[FT_GRID_CELLS] - gs[0];
            S.counts[0] = min(total, S.cap1);
            S.counts[1] = min(n2, S.cap2);
            S.counts[2] = (total > S.cap1 || n2 > S.cap2) ? 1 : 0;
        }
        return;
    }
    const int base = gs[0], n2 = min(gs[FT_GRID_CELLS] - base, S.cap2);
    const int p = ((int)blockIdx.x - 1) * FT_INIT_PREP_T + tid;  // position behind `base`
    if (p >= n2) return;
    const float4 *rec = S.F2.gridRec[0];
    const float4 me = rec[base + p];
    const int idx = __float_as_int(me.w) & 0xffffff;
    const int c = init_cell_of(S.F2, me.x, me.y);
    int ord = p;
    if (c >= 0) {
        const int b = gs[c], e = gs[c + 1];
        int smaller = 0;
        for (int q = b; q < e; q++) smaller += (__float_as_int(rec[q].w) & 0xffffff) < idx ? 1 : 0;
        ord = b - base + smaller;
    }
    S.ordOfPos[p] = ord;
    if (ord >= 0 && ord < S.cap2) S.idxOfOrd[ord] = idx;
}

// c joins the ascending t[0 .. FT_INIT_TOP)
__device__ __forceinline__ void top_insert(unsigned t[FT_INIT_TOP], unsigned c) {
#pragma unroll
    for (int k = 0; k < FT_INIT_TOP; k++) {
        const unsigned lo = min(t[k], c);
        c = max(t[k], c);
        t[k] = lo;
    }
}

// A wave per row.  The window of Frame::GetFeaturesInArea(x, y, windowSize, 0, 0) (src/Frame.cc:681-747) in octave 0 of F2's
// grid: one lane per column of cells (a column's cells minCY .. maxCY are one contiguous range of entries, at most 64
// columns), a wave scan lays the ranges end to end and the lanes take the entries 64 at a time.
#define FT_INIT_WPB 4
__global__ __launch_bounds__(64 * FT_INIT_WPB) void k_init_candidates(FtInitSearch S) {
    const int lane = threadIdx.x & 63;
    const int row = (int)blockIdx.x * FT_INIT_WPB + wave_index();
    const int n1 = __builtin_amdgcn_readfirstlane(S.counts[0]), n2 = __builtin_amdgcn_readfirstlane(S.counts[1]);
    if (row >= n1) return;
    const int i1 = __builtin_amdgcn_readfirstlane(S.rows[row]);
    const float x = S.prev[2 * (size_t)i1], y = S.prev[2 * (size_t)i1 + 1], r = S.window;
    unsigned long long d1[4];
    load_desc256(S.desc1, i1, d1);
    const FtDevFrame &F = S.F2;
    const int *gs = F.gridStart[0];
    const float4 *rec = F.gridRec[0];
    const uint4 *gd = (const uint4 *)F.gridDesc[0];
    const int base = gs[0];
    unsigned *seg = S.seg + (size_t)row * (size_t)S.cap2;
    unsigned t[FT_INIT_TOP];
#pragma unroll
    for (int k = 0; k < FT_INIT_TOP; k++) t[k] = FT_INIT_NONE;
    int count = 0;
    const Window w = cell_window(F, x, y, r);
    if (!w.empty && n2 > 0) {
        const int ncols = w.maxCX - w.minCX + 1;  // 1 .. 64
        int b = 0, cnt = 0;
        if (lane < ncols) {
            const int *col = gs + (w.minCX + lane) * FT_GRID_ROWS;
            b = col[w.minCY];
            cnt = col[w.maxCY + 1] - b;
        }
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        const int total = __builtin_amdgcn_readlane(incl, 63);
        for (int t0 = 0; t0 < total; t0 += 64) {
            const int e = min(t0 + lane, total - 1);
            int c = 0;  // the column entry e falls into: the number of columns that end at or before it
            for (int k = 0; k < ncols - 1; k++) c += e >= __builtin_amdgcn_readlane(incl, k) ? 1 : 0;
            const int pos = __shfl(b, c) + (e - (__shfl(incl, c) - __shfl(cnt, c)));
            const int p = min(max(pos - base, 0), n2 - 1);  // (n2 >= 1 here: the window holds entries)
            const float4 kp = rec[base + p];
            const uint4 a0 = gd[2 * (size_t)(base + p)], a1 = gd[2 * (size_t)(base + p) + 1];
            const unsigned ord = (unsigned)S.ordOfPos[p];
            // level band [0, 0] and the box of GetFeaturesInArea (:722-737); the cell tests are the ranges walked
            bool cand = t0 + lane < total && pos - base == p && (__float_as_int(kp.w) >> 24) == 0;
            cand = cand && fabsf(__fsub_rn(kp.x, x)) < r && fabsf(__fsub_rn(kp.y, y)) < r;
            const unsigned long long d2[4] = {(unsigned long long)a0.x | ((unsigned long long)a0.y << 32),
                                              (unsigned long long)a0.z | ((unsigned long long)a0.w << 32),
                                              (unsigned long long)a1.x | ((unsigned long long)a1.y << 32),
                                              (unsigned long long)a1.z | ((unsigned long long)a1.w << 32)};
            const int dist = __popcll(d1[0] ^ d2[0]) + __popcll(d1[1] ^ d2[1]) + __popcll(d1[2] ^ d2[2]) + __popcll(d1[3] ^ d2[3]);
            const unsigned word = ((unsigned)dist << FT_INIT_ORD_BITS) | (ord & FT_INIT_ORD_MASK);
            const unsigned long long m = __ballot(cand);
            if (cand) {
                const int at = count + __popcll(m & ((1ull << lane) - 1ull));
                if (at < S.cap2) seg[at] = word;
                top_insert(t, word);
            }
            count += __popcll(m);
        }
    }
    // the FT_INIT_TOP smallest words of the wave: the lanes' lists are ascending, so the wave's minimum is some lane's head
    unsigned out = FT_INIT_NONE;
#pragma unroll
    for (int k = 0; k < FT_INIT_TOP; k++) {
        const unsigned m = wave_min_u32(t[0]);
        if (lane == k) out = m;
        if (t[0] == m && m != FT_INIT_NONE) {  // (words are unique inside a row: one lane pops)
#pragma unroll
            for (int j = 0; j + 1 < FT_INIT_TOP; j++) t[j] = t[j + 1];
            t[FT_INIT_TOP - 1] = FT_INIT_NONE;
        }
    }
    if (lane < FT_INIT_TOP) S.top[(size_t)row * FT_INIT_TOP + lane] = out;
    if (lane == 0) S.segCount[row] = min(count, S.cap2);
}

// LDS: state[ord] = vMatchedDistance << 16 | row of vnMatches21 (0xffff / 0xffff = INT_MAX / -1), then rowMatch[row] = the ord
// the row holds, -1 = never matched, -2 - ord = evicted from ord (what its rotation bin was computed with).
#define FT_INIT_RES_T 1024
#define FT_INIT_FREE 0xffffffffu
__global__ __launch_bounds__(FT_INIT_RES_T) void k_init_resolve(FtInitSearch S) {
    extern __shared__ unsigned ini_lds[];
    __shared__ int ini_nm;
    const int tid = threadIdx.x, lane = tid & 63;
    const int n1 = __builtin_amdgcn_readfirstlane(S.counts[0]), n2 = __builtin_amdgcn_readfirstlane(S.counts[1]);
    unsigned *state = ini_lds;
    int *rowMatch = (int *)(ini_lds + S.cap2);
    for (int o = tid; o < n2; o += FT_INIT_RES_T) state[o] = FT_INIT_FREE;
    for (int r = tid; r < n1; r += FT_INIT_RES_T) rowMatch[r] = -1;
    if (tid == 0) ini_nm = 0;
    // what the reference leaves for a keypoint that is no row or ends unmatched; the rows overwrite theirs at the end
    for (int i = tid; i < S.N1; i += FT_INIT_RES_T) {
        S.matches12[i] = -1;
        S.prevOut[2 * (size_t)i] = S.prev[2 * (size_t)i];
        S.prevOut[2 * (size_t)i + 1] = S.prev[2 * (size_t)i + 1];
    }
    if (S.matchedDist)
        for (int i = tid; i < S.F2.N; i += FT_INIT_RES_T) S.matchedDist[i] = INT_MAX;
    __threadfence();
    __syncthreads();
    if (tid < 64) {  // the sequential walk over the rows, wave 0; everything below is wave-uniform
        const uint4 *top4 = (const uint4 *)S.top;
        uint4 nextTop = make_uint4(FT_INIT_NONE, FT_INIT_NONE, FT_INIT_NONE, FT_INIT_NONE);
        int nextCnt = 0;
        if (lane < n1) {
            nextTop = top4[lane];
            nextCnt = S.segCount[lane];
        }
        for (int r0 = 0; r0 < n1; r0 += 64) {
            const uint4 curTop = nextTop;
            const int curCnt = nextCnt;
            if (r0 + 64 + lane < n1) {  // the next 64 rows are on their way while these are decided
                nextTop = top4[r0 + 64 + lane];
                nextCnt = S.segCount[r0 + 64 + lane];
            }
            const int nr = min(64, n1 - r0);
            for (int j = 0; j < nr; j++) {
                const int row = r0 + j;
                const unsigned k[FT_INIT_TOP] = {(unsigned)__builtin_amdgcn_readlane((int)curTop.x, j), (unsigned)__builtin_amdgcn_readlane((int)curTop.y, j),
                                                 (unsigned)__builtin_amdgcn_readlane((int)curTop.z, j), (unsigned)__builtin_amdgcn_readlane((int)curTop.w, j)};
                const int cnt = __builtin_amdgcn_readlane(curCnt, j);
                if (cnt <= 0) continue;  // vIndices2.empty() (:769)
                unsigned best = FT_INIT_NONE, second = FT_INIT_NONE;
                int found = 0;
#pragma unroll
                for (int q = 0; q < FT_INIT_TOP; q++) {
                    if (k[q] == FT_INIT_NONE) continue;
                    const unsigned held = state[min(k[q] & FT_INIT_ORD_MASK, (unsigned)(n2 - 1))] >> 16;
                    const bool free_ = held > (k[q] >> FT_INIT_ORD_BITS);  // not `vMatchedDistance[i2] <= dist` (:786)
                    if (free_ && found == 0) best = k[q];
                    else if (free_ && found == 1) second = k[q];
                    found += free_ ? 1 : 0;
                }
                const bool complete = cnt <= FT_INIT_TOP;
                // the top record does not decide the row: too few of it are free, more candidates exist, and the best (if any)
                // would pass TH_LOW - best and second best from the row's segment
                if (!complete && (found == 0 || (found == 1 && (int)(best >> FT_INIT_ORD_BITS) <= FT_INIT_TH_LOW))) {
                    const unsigned *seg = S.seg + (size_t)row * (size_t)S.cap2;
                    unsigned k0 = FT_INIT_NONE, k1 = FT_INIT_NONE;
                    for (int e = lane; e < cnt; e += 64) {
                        const unsigned word = seg[e];
                        const unsigned held = state[min(word & FT_INIT_ORD_MASK, (unsigned)(n2 - 1))] >> 16;
                        if (held <= (word >> FT_INIT_ORD_BITS)) continue;
                        const unsigned larger = max(word, k0);
                        k0 = min(word, k0);
                        k1 = min(larger, k1);
                    }
                    best = wave_min_u32(k0);
                    second = wave_min_u32(k0 == best ? k1 : k0);
                }
                if (best == FT_INIT_NONE) continue;
                const int bestDist = (int)(best >> FT_INIT_ORD_BITS);
                if (bestDist > FT_INIT_TH_LOW) continue;
                // bestDist < (float)bestDist2 * mfNNratio (:803), bestDist2 = INT_MAX without a second candidate
                const float second2 = second == FT_INIT_NONE ? (float)INT_MAX : (float)(int)(second >> FT_INIT_ORD_BITS);
                if (!((float)bestDist < __fmul_rn(second2, S.nnRatio))) continue;
                const unsigned ord = min(best & FT_INIT_ORD_MASK, (unsigned)(n2 - 1));
                const unsigned owner = state[ord] & 0xffffu;
                if (lane == 0) {
                    if (owner != 0xffffu) rowMatch[owner] = -2 - (int)ord;  // vnMatches12[vnMatches21[bestIdx2]] = -1 (:807)
                    rowMatch[row] = (int)ord;
                    state[ord] = ((unsigned)bestDist << 16) | (unsigned)row;
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    __syncthreads();
    const FtDevFrame &F = S.F2;
    auto bin_of_row = [&](int r, int m) -> int {
        const int ord = m >= 0 ? m : -2 - m;
        return init_bin(S.keys1[S.rows[r]].angle, F.keys[S.idxOfOrd[ord]].angle);
    };
    // a row that was evicted (-2 - ord) stays in the bin it was filed under (:807 clears vnMatches12, not rotHist)
    const int keep = rot_filter_keep<FT_INIT_RES_T>(n1, S.checkOrientation, [&](int r) {
        const int m = rowMatch[r];
        return m == -1 ? -1 : bin_of_row(r, m);
    });
    int nm = 0;
    for (int r = tid; r < n1; r += FT_INIT_RES_T) {
        const int m = rowMatch[r];
        if (m < 0) continue;
        if (S.checkOrientation) {
            const int bin = bin_of_row(r, m);
            if (bin >= 0 && bin < FT_HISTO_LENGTH && !((keep >> bin) & 1)) continue;  // removed (:839-852)
        }
        const int i1 = S.rows[r], i2 = S.idxOfOrd[m];
        S.matches12[i1] = i2;
        S.prevOut[2 * (size_t)i1] = F.keys[i2].x;  // vbPrevMatched[i1] = F2.mvKeysUn[vnMatches12[i1]].pt (:857-859)
        S.prevOut[2 * (size_t)i1 + 1] = F.keys[i2].y;
        nm++;
    }
    if (S.matchedDist)  // vMatchedDistance keeps the distance of a match the histogram removed
        for (int o = tid; o < n2; o += FT_INIT_RES_T) {
            const unsigned s = state[o];
            if (s != FT_INIT_FREE) S.matchedDist[S.idxOfOrd[o]] = (int)(s >> 16);
        }
    nm = wave_sum_i32(nm);
    if (lane == 0 && nm) atomicAdd(&ini_nm, nm);
    __syncthreads();
    if (tid == 0) *S.nMatches = ini_nm;
}

}  // namespace

int ft_launch_init_prepare(hipStream_t st, const FtInitSearch &S) {
    hipLaunchKernelGGL(k_init_prepare, dim3(1 + (S.cap2 + FT_INIT_PREP_T - 1) / FT_INIT_PREP_T), dim3(FT_INIT_PREP_T), 0, st, S);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_init_candidates(hipStream_t st, const FtInitSearch &S) {
    hipLaunchKernelGGL(k_init_candidates, dim3(std::max(1, (S.cap1 + FT_INIT_WPB - 1) / FT_INIT_WPB)), dim3(64 * FT_INIT_WPB), 0, st, S);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_init_resolve(hipStream_t st, const FtInitSearch &S) {
    const size_t lds = sizeof(unsigned) * ((size_t)S.cap1 + (size_t)S.cap2);
    if (lds > FT_INIT_MAX_LDS) {
        ft_set_error("SearchForInitialization: the level-0 keypoints of the two frames exceed the LDS tables of the resolution");
        return FT_ERR_CAPACITY;
    }
    const int rc = ft_allow_max_lds<k_init_resolve>();
    if (rc != FT_OK) return rc;
    hipLaunchKernelGGL(k_init_resolve, dim3(1), dim3(FT_INIT_RES_T), lds, st, S);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

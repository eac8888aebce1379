// HIP kernels of the KeyFrameDatabase queries (reference src/KeyFrameDatabase.cc:604-730 DetectNBestCandidates, :733-845
// DetectRelocalizationCandidates, up to the scores; Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68 L1Scoring::score) for gfx950
// (wave64).  A query is TWO launches whatever the number of stored keyframes or words: k_kfdb_count, then k_kfdb_score.
// The reference walks an inverted file because it is sequential; here a wave takes a stored keyframe (a ROW) and intersects
// its sorted word ids with the query's, which sit in the LDS: a lane holds one stored id of each of four chunks of 64 and
// binary-searches the four among the query's side by side, a ballot gives the shared words of a chunk.  Both kernels run the
// same grid: workgroups of sixteen waves, the waves stride over the rows.
//   k_kfdb_count  the number of shared words and the smallest shared word of a row; then the row's state rule (:623-633, resp.
//                 :748-754), applied once per row for all its shared words: a row whose stamp differs from the query id has
//                 its count reset and - unless it is connected - is stamped and LISTED; the count grows by the shared words
//                 (a connected row is reset at every word: it ends with 1).  A listed row files its first shared word in
//                 `first` (the list order of the reference is ascending (first shared word, insertion order)), counts itself
//                 and brings its count into the call's maximum (LDS atomics, then one pair of atomics per workgroup on the
//                 call slot; neither the sum nor the maximum depends on the order).
//   k_kfdb_score  minCommonWords = (int)(maxCommonWords * 0.8f) from the call slot; a listed row with more words than that is
//                 scored: per chunk the lanes with a shared word load both values and form (|vi - wi| - |vi|) - |wi|, and the
//                 terms are added one after the other in lane order = ascending word order into ONE double (a uniform loop over
//                 the ballot's bits, the term read with two v_readlane) - no tree, no DPP reduction.  The terms hold no
//                 product, so nothing can be contracted.  -sum / 2.0, the rounding to float, the float into the row's state;
//                 the row takes the next record of the call (atomic counter: the host orders the records).
//   k_kfdb_move   copies the words of the live rows into new storage (growth by doubling, compaction): a workgroup per row.
// Every result is written with plain vector stores.
#include <algorithm>

#include "ft_internal.h"
#include "ft_search.h"
#include "wave_ops.h"

namespace {

#define FT_KFDB_T 1024        // sixteen waves share the query in the LDS and ONE pair of atomics on the call slot
#define FT_KFDB_MAX_GRID 512  // workgroups of a query: beyond 8 192 rows the waves stride

#define FT_KFDB_U 4  // chunks of 64 stored words a wave has in flight: their loads and their searches are independent

// Index of id[u] among the n >= 1 ascending ids q (LDS), or -1, for the lane's FT_KFDB_U words at once: the searches take the
// same number of steps (enough to halve [0, n] down to a point), so their LDS reads overlap instead of waiting for each other.
__device__ __forceinline__ void find_words(const unsigned *q, int n, const unsigned (&id)[FT_KFDB_U], int (&pos)[FT_KFDB_U]) {
    int lo[FT_KFDB_U], hi[FT_KFDB_U];
#pragma unroll
    for (int u = 0; u < FT_KFDB_U; u++) lo[u] = 0, hi[u] = n;
    for (int s = 32 - __clz(n); s > 0; s--) {
#pragma unroll
        for (int u = 0; u < FT_KFDB_U; u++) {
            const int mid = (lo[u] + hi[u]) >> 1;
            const bool open = lo[u] < hi[u], less = q[min(mid, n - 1)] < id[u];
            lo[u] = open && less ? mid + 1 : lo[u];
            hi[u] = open && !less ? mid : hi[u];
        }
    }
#pragma unroll
    for (int u = 0; u < FT_KFDB_U; u++) pos[u] = lo[u] < n && q[min(lo[u], n - 1)] == id[u] ? lo[u] : -1;
}

// the lane's words of the chunks at c, c + 64, ...: FT_KFDB_NOT_LISTED (which no query holds) behind the row's end
__device__ __forceinline__ void load_words(const unsigned *ids, size_t start, int len, int c, int lane, unsigned (&id)[FT_KFDB_U]) {
#pragma unroll
    for (int u = 0; u < FT_KFDB_U; u++) {
        const int i = c + 64 * u + lane;
        id[u] = i < len ? ids[start + i] : FT_KFDB_NOT_LISTED;
    }
}

__device__ __forceinline__ void load_query(const FtKfdbCall &T, unsigned *sq) {
    const unsigned *q = (const unsigned *)(T.arena + T.qIds);
    for (int i = threadIdx.x; i < T.nQuery; i += FT_KFDB_T) sq[i] = q[i];
    __syncthreads();
}

__device__ __forceinline__ bool is_connected(const int *rows, int n, int row) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rows[mid] < row) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && rows[lo] == row;
}

__global__ __launch_bounds__(FT_KFDB_T) void k_kfdb_count(const FtKfdbCall T) {
    __shared__ unsigned sq[FT_KFDB_MAX_QUERY_WORDS];
    load_query(T, sq);
    const int lane = threadIdx.x & 63;
    const int nWaves = gridDim.x * (FT_KFDB_T / 64);
    unsigned *first = (unsigned *)(T.arena + T.first);
    int *slot = (int *)(T.arena + T.slot);
    // the workgroup's listed rows and their largest count: atomics of thousands of waves on the two words of the call slot
    // took longer than the intersections (3 800 listed rows: 100 us); the LDS takes them, the slot one pair per workgroup
    __shared__ int sListed, sMax;
    if (threadIdx.x == 0) sListed = sMax = 0;
    __syncthreads();
    for (int row = blockIdx.x * (FT_KFDB_T / 64) + wave_index(); row < T.nRows; row += nWaves) {
        const int len = __builtin_amdgcn_readfirstlane(T.rowLen[row]);
        const unsigned start = __builtin_amdgcn_readfirstlane(T.rowStart[row]);
        int count = 0;
        unsigned mine = FT_KFDB_NOT_LISTED;  // the smallest shared word this lane has seen
        for (int c = 0; c < len; c += 64 * FT_KFDB_U) {
            unsigned id[FT_KFDB_U];
            int pos[FT_KFDB_U];
            load_words(T.ids, start, len, c, lane, id);
            find_words(sq, T.nQuery, id, pos);
#pragma unroll
            for (int u = 0; u < FT_KFDB_U; u++) {
                if (pos[u] >= 0) mine = min(mine, id[u]);
                count += __popcll(__ballot(pos[u] >= 0));
            }
        }
        unsigned listed = FT_KFDB_NOT_LISTED;
        if (count > 0) {  // (wave-uniform)
            const unsigned firstWord = wave_min_u32(mine);
            if (lane == 0) {
                FtKfdbState S = T.state[row];
                if (S.stamp != T.queryId) {
                    S.words = 0;
                    if (!is_connected((const int *)(T.arena + T.connected), T.nConnected, row)) {
                        S.stamp = T.queryId;
                        S.words = count;
                        listed = firstWord;
                    } else S.words = 1;  // reset at every shared word, then incremented
                } else S.words += count;
                T.state[row] = S;
                if (listed != FT_KFDB_NOT_LISTED) {
                    atomicAdd(&sListed, 1);
                    atomicMax(&sMax, S.words);
                }
            }
        }
        if (lane == 0) first[row] = listed;
    }
    __syncthreads();  // (no thread leaves the row loop early)
    if (threadIdx.x == 0 && sListed > 0) {
        atomicAdd(&slot[0], sListed);
        if (sMax > __atomic_load_n(&slot[1], __ATOMIC_RELAXED)) atomicMax(&slot[1], sMax);  // (a stale read only costs the atomic)
    }
}

__global__ __launch_bounds__(FT_KFDB_T) void k_kfdb_score(const FtKfdbCall T) {
    __shared__ unsigned sq[FT_KFDB_MAX_QUERY_WORDS];
    load_query(T, sq);
    const int lane = threadIdx.x & 63;
    const int nWaves = gridDim.x * (FT_KFDB_T / 64);
    const unsigned *first = (const unsigned *)(T.arena + T.first);
    const double *qv = (const double *)(T.arena + T.qVals);
    int *slot = (int *)(T.arena + T.slot);
    const int maxCommonWords = slot[1];
    const int minCommonWords = (int)(maxCommonWords * 0.8f);
    for (int row = blockIdx.x * (FT_KFDB_T / 64) + wave_index(); row < T.nRows; row += nWaves) {
        const unsigned firstWord = __builtin_amdgcn_readfirstlane(first[row]);
        if (firstWord == FT_KFDB_NOT_LISTED) continue;
        const int words = __builtin_amdgcn_readfirstlane(T.state[row].words);
        if (!(words > minCommonWords)) continue;
        const int len = __builtin_amdgcn_readfirstlane(T.rowLen[row]);
        const unsigned start = __builtin_amdgcn_readfirstlane(T.rowStart[row]);
        double sum = 0;
        for (int c = 0; c < len; c += 64 * FT_KFDB_U) {
            unsigned id[FT_KFDB_U];
            int pos[FT_KFDB_U];
            load_words(T.ids, start, len, c, lane, id);
            find_words(sq, T.nQuery, id, pos);
#pragma unroll
            for (int u = 0; u < FT_KFDB_U; u++) {  // chunk after chunk, and inside a chunk lane after lane: ascending words
                double term = 0;
                if (pos[u] >= 0) {
                    const double vi = qv[pos[u]], wi = T.vals[(size_t)start + c + 64 * u + lane];  // v1 is the query, v2 the stored keyframe (:662)
                    term = (fabs(vi - wi) - fabs(vi)) - fabs(wi);
                }
                unsigned long long mask = __ballot(pos[u] >= 0);
                const unsigned long long bits = (unsigned long long)__double_as_longlong(term);
                while (mask) {
                    const int l = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)bits, l);
                    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(bits >> 32), l);
                    sum += __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
                }
            }
        }
        if (lane == 0) {
            const double score = -sum / 2.0;
            const float si = (float)score;
            T.state[row].score = si;
            const int k = atomicAdd(&slot[2], 1);  // k < nRows: a row is scored once
            FtKfdbRec R;
            R.row = row;
            R.first = (int)firstWord;
            R.words = words;
            R.score = si;
            ((FtKfdbRec *)(T.arena + T.recs))[k] = R;
            ((double *)(T.arena + T.raw))[k] = score;
        }
    }
}

__global__ __launch_bounds__(FT_KFDB_T) void k_kfdb_move(const unsigned *oldIds, const double *oldVals, const unsigned *oldStart,
                                                         const int *map, unsigned *newIds, double *newVals, const unsigned *newStart,
                                                         const int *newLen) {
    const int row = blockIdx.x;
    const size_t from = oldStart[map[row]], to = newStart[row];
    const int len = newLen[row];
    for (int i = threadIdx.x; i < len; i += FT_KFDB_T) {
        newIds[to + i] = oldIds[from + i];
        newVals[to + i] = oldVals[from + i];
    }
}

int kfdbGrid(int nRows) { return std::min((nRows + FT_KFDB_T / 64 - 1) / (FT_KFDB_T / 64), FT_KFDB_MAX_GRID); }

}  // namespace

int ft_launch_kfdb_count(hipStream_t st, const FtKfdbCall &T) {
    hipLaunchKernelGGL(k_kfdb_count, dim3((unsigned)kfdbGrid(T.nRows)), dim3(FT_KFDB_T), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_kfdb_score(hipStream_t st, const FtKfdbCall &T) {
    hipLaunchKernelGGL(k_kfdb_score, dim3((unsigned)kfdbGrid(T.nRows)), dim3(FT_KFDB_T), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_kfdb_move(hipStream_t st, const unsigned *oldIds, const double *oldVals, const unsigned *oldStart, const int *map,
                        unsigned *newIds, double *newVals, const unsigned *newStart, const int *newLen, int nRows) {
    hipLaunchKernelGGL(k_kfdb_move, dim3((unsigned)nRows), dim3(FT_KFDB_T), 0, st, oldIds, oldVals, oldStart, map, newIds, newVals,
                       newStart, newLen);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

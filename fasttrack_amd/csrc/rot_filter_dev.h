// The rotation-consistency filter of the matchers on the device (reference src/ORBmatcher.cc: the rotHist blocks of every
// Search*, ComputeThreeMaxima :2210-2251), by ONE workgroup of THREADS threads over n rows: the device twin of rot_hist.h.
// What differs between the matchers - which rows are filed and where a row's two angles come from, in which order - is the
// caller's functor; init_bin and three_maxima_keep (ft_search.h) are the arithmetic.  Device only.
#pragma once
#include "ft_search.h"
#include "wave_ops.h"

// The bins to keep, as three_maxima_keep returns them, in every thread; all ones without `check`.  binOf(i) = the bin of row i,
// -1 = the row is not filed (a bin outside the histogram is one the reference asserts against: not filed either).  Called by
// every thread of the workgroup, once per kernel; the rows' entries must be visible to the workgroup on entry.  Its first barrier
// (behind the zeroing of the histogram) is passed with or without `check`.
template <int THREADS, class BinOf>
__device__ __forceinline__ int rot_filter_keep(int n, int check, BinOf binOf) {
    __shared__ int hist[FT_HISTO_LENGTH];
    __shared__ int keepBits;
    const int tid = threadIdx.x;
    if (tid < FT_HISTO_LENGTH) hist[tid] = 0;
    __syncthreads();
    if (!check) return -1;
    for (int i = tid; i < n; i += THREADS) {
        const int bin = binOf(i);
        if (bin >= 0 && bin < FT_HISTO_LENGTH) atomicAdd(&hist[bin], 1);
    }
    __syncthreads();
    if (tid == 0) keepBits = three_maxima_keep(hist);
    __syncthreads();
    return keepBits;
}

// The filter on a row of matches (matches[i] = the match of feature i, < 0: none): the matches outside the kept bins become -1,
// *out = the number that stay.  binOfMatch(i, m) = the bin of the match i -> m.
template <int THREADS, class BinOfMatch>
__device__ __forceinline__ void rot_filter_rows(int *matches, int n, int check, int *out, BinOfMatch binOfMatch) {
    __shared__ int total;
    const int tid = threadIdx.x;
    if (tid == 0) total = 0;
    const int keep = rot_filter_keep<THREADS>(n, check, [&](int i) {
        const int m = matches[i];
        return m < 0 ? -1 : binOfMatch(i, m);
    });
    int nm = 0;
    for (int i = tid; i < n; i += THREADS) {
        const int m = matches[i];
        if (m < 0) continue;
        if (check) {
            const int bin = binOfMatch(i, m);
            if (bin >= 0 && bin < FT_HISTO_LENGTH && !((keep >> bin) & 1)) {
                matches[i] = -1;
                continue;
            }
        }
        nm++;
    }
    nm = wave_sum_i32(nm);
    if ((tid & 63) == 0 && nm) atomicAdd(&total, nm);
    __syncthreads();
    if (tid == 0) *out = total;
}

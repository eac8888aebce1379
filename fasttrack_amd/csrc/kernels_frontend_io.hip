// HIP kernels that move a front end's frames and results between pinned host memory and HBM (gfx950, wave64): each replaces a
// handful of small copies through the DMA queue - a few microseconds of work behind tens of microseconds of latency - by one
// launch.  They match nothing and extract nothing; the reference has no counterpart but the order of k_deliver_ordered's output.
//   k_upload           the frames of a small batch into level 0 of the slot pyramids           (ft_extract_prepare, extractor.cpp)
//   k_deliver          every result of a small batch and its counters: one camera (ft_extract_batch, extractor.cpp), or both
//                      and the stereo outputs (frontendEnqueue, stereo_frontend.cpp)
//   k_deliver_ordered  ft_extract_batch's results in the order ORBextractor::operator() returns them (reference src/ORBextractor.cc:1466-1487)
//   k_finish_counts    the end-of-batch counters of an extractor                               (ft_extract_finish_counts, extractor.cpp)
// The deliveries of a tracked batch (k_deliver_blocks, k_deliver_batch, k_gather_batch): kernels_frame.hip.
#include "ft_internal.h"

namespace {

__global__ __launch_bounds__(256) void k_upload(const FtSrcEntry *srcTab, int width, int height, uint8_t *slot0, int pitch,
                                                size_t slotBytes, const uint8_t **l0Table) {
    const int slot = blockIdx.y;
    const FtSrcEntry e = srcTab[slot];  // (pinned host memory, written by the host just before the launch or replay)
    const uint8_t *src = e.ptr;
    const size_t sstride = (size_t)e.stride;
    uint8_t *dst = slot0 + (size_t)slot * slotBytes;
    const int t = blockIdx.x * 256 + threadIdx.x, T = gridDim.x * 256;
    if ((width & 3) == 0 && (((uintptr_t)src | sstride) & 3) == 0) {  // dword columns (the slot pitch is a multiple of 64 bytes)
        const int wq = width >> 2, n = wq * height;
        for (int i = t; i < n; i += T) {
            const int y = i / wq, x = i - y * wq;
            ((unsigned *)(dst + (size_t)y * pitch))[x] = ((const unsigned *)(src + (size_t)y * sstride))[x];
        }
    } else {
        const int n = width * height;
        for (int i = t; i < n; i += T) {
            const int y = i / width, x = i - y * width;
            dst[(size_t)y * pitch + x] = src[(size_t)y * sstride + x];
        }
    }
    if (t == 0) l0Table[slot] = dst;
}

// grid (DL_BLOCKS, batch): the blocks of an image share the rows of its six result arrays dword by dword (every record
// size is a multiple of four bytes); the stores go over the host link, the counters with them
#define DL_BLOCKS 24
__global__ __launch_bounds__(256) void k_deliver(FtDeliverArgs a) {
    const int slot = blockIdx.y;
    const int nl = a.nL[slot], nr = a.nR ? a.nR[slot] : 0;  // one camera only: the right-hand pointers are null
    const int t = blockIdx.x * 256 + threadIdx.x, T = DL_BLOCKS * 256;
    auto rows = [&](const void *src, void *dst, int recBytes, int n) {
        if (!dst || n <= 0) return;
        const unsigned *s = (const unsigned *)((const uint8_t *)src + (size_t)slot * a.srcStride * recBytes);
        unsigned *d = (unsigned *)((uint8_t *)dst + (size_t)slot * a.dstStride * recBytes);
        const int words = n * (recBytes >> 2);
        for (int i = t; i < words; i += T) d[i] = s[i];
    };
    rows(a.keysL, a.oKeysL, (int)sizeof(ft_keypoint), nl);
    rows(a.descL, a.oDescL, 32, nl);
    rows(a.uright, a.oUright, 4, nl);
    rows(a.depth, a.oDepth, 4, nl);
    rows(a.keysR, a.oKeysR, (int)sizeof(ft_keypoint), nr);
    rows(a.descR, a.oDescR, 32, nr);
    if (t == 0) {
        a.oNL[slot] = nl;
        if (a.oNR) a.oNR[slot] = nr;
        if (a.oNMatches) a.oNMatches[slot] = a.nMatches[slot];
        if (slot == 0) {
            *a.oOverflowL = *a.overflowL;
            if (a.oOverflowR) *a.oOverflowR = *a.overflowR;
        }
    }
}

// The results of ft_extract_batch in the order ORBextractor::operator() returns them (src/ORBextractor.cc:1466-1487: keypoints
// outside the lapping area fill the output from the front, those inside it from the back), written straight into the caller's
// arrays in pinned host memory: a workgroup per image, the position of a keypoint from a running count of the lapping-area
// keypoints in front of it (ballots, wave totals through LDS).  Replaces the copy of whole rows into the library's staging and
// the host's pass over them (ft_extract_batch: 2 x 15 MB per 128 two-camera frames of 2 000 features, through the context's
// host threads).  An image with more keypoints than the caller's rows hold is left alone (the host reports FT_ERR_CAPACITY).
__global__ __launch_bounds__(256) void k_deliver_ordered(FtOrderedArgs a) {
    const int slot = a.b0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.nSel[slot];
    __shared__ int wcnt[2][4];
    if (n > a.capacity) {
        if (tid == 0) a.oMono[slot] = 0;
        return;
    }
    const unsigned *src = (const unsigned *)(a.keys + (size_t)slot * a.srcStride);
    const uint4 *sd = (const uint4 *)(a.desc + (size_t)slot * a.srcStride * 32);
    unsigned *dk = a.oKeys ? (unsigned *)(a.oKeys + (size_t)slot * a.capacity) : nullptr;
    uint4 *dd = a.oDesc ? (uint4 *)(a.oDesc + (size_t)slot * a.capacity * 32) : nullptr;
    constexpr int W = (int)sizeof(ft_keypoint) / 4;
    int lapBefore = 0;
    for (int base = 0, r = 0; base < n; base += 256, r ^= 1) {  // (uniform)
        const int i = base + tid;
        const bool real = i < n;
        unsigned kw[W];
#pragma unroll
        for (int k = 0; k < W; k++) kw[k] = real ? src[(size_t)i * W + k] : 0u;
        const float x = __uint_as_float(kw[0]);  // ft_keypoint::x is the first field
        const bool inLap = real && x >= a.lap0 && x <= a.lap1;
        const unsigned long long bal = __ballot(inLap);
        if (lane == 0) wcnt[r][wave] = __popcll(bal);
        __syncthreads();  // (two buffers: the next round's writes cannot pass a reader of this one)
        int below = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            below += w < wave ? wcnt[r][w] : 0;
            total += wcnt[r][w];
        }
        if (real) {
            const int rankLap = lapBefore + below + __popcll(bal & ((1ull << lane) - 1ull));
            const int dst = inLap ? n - 1 - rankLap : i - rankLap;
            if (dk) {
#pragma unroll
                for (int k = 0; k < W; k++) dk[(size_t)dst * W + k] = kw[k];
            }
            if (dd) {
                dd[2 * (size_t)dst] = sd[2 * (size_t)i];
                dd[2 * (size_t)dst + 1] = sd[2 * (size_t)i + 1];
            }
        }
        lapBefore += total;
    }
    if (tid == 0) a.oMono[slot] = n - lapBefore;
}

// the counters the host reads at the end of a wide batch - per-image totals, the overflow flag, the demand of the octree tiers
// behind k_octree (reset here for the next batch) - written to pinned host memory by ONE small kernel: they were six or seven
// 4-byte copies and two fills through the DMA queue, ~18 us of link latency each, one after the other at the tail of every
// ft_extract_batch / front-end batch
__global__ __launch_bounds__(256) void k_finish_counts(FtCountsArgs a) {
    for (int i = threadIdx.x; i < a.batch; i += 256) a.oNSel[i] = a.nSel[i];
    if (threadIdx.x == 0) *a.oOverflow = *a.overflow;
    if (a.bigCount && (int)threadIdx.x < a.nStreams) {
        const int k = threadIdx.x;
        a.oHist[k] = a.bigCount[4 * k + 2];
        a.oBig[k] = a.bigCount[4 * k + 3];
        a.bigCount[4 * k + 2] = 0;
        a.bigCount[4 * k + 3] = 0;
    }
}

}  // namespace

int ft_launch_upload(hipStream_t st, int batch, const FtSrcEntry *srcTab, int width, int height, uint8_t *slot0, int pitch,
                     size_t slotBytes, const uint8_t **l0Table) {
    hipLaunchKernelGGL(k_upload, dim3(48, batch), dim3(256), 0, st, srcTab, width, height, slot0, pitch, slotBytes, l0Table);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_deliver(hipStream_t st, int batch, const FtDeliverArgs &a) {
    hipLaunchKernelGGL(k_deliver, dim3(DL_BLOCKS, batch), dim3(256), 0, st, a);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_deliver_ordered(hipStream_t st, int nb, const FtOrderedArgs &a) {
    if (nb <= 0) return FT_OK;
    hipLaunchKernelGGL(k_deliver_ordered, dim3(nb), dim3(256), 0, st, a);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_finish_counts(hipStream_t st, const FtCountsArgs &a) {
    hipLaunchKernelGGL(k_finish_counts, dim3(1), dim3(256), 0, st, a);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

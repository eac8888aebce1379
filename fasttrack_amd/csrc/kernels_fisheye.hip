// HIP kernels of Frame::ComputeStereoFishEyeMatches for gfx950 (wave64), for one frame and for every frame of a tracked batch:
// brute-force Hamming on 256-bit descriptors, minima on packed (distance, index) keys so ties resolve exactly like the
// reference's sequential "dist < bestDist" scans.
//   k_fisheye_2nn, k_fisheye_2nn_batch                  BFMatcher knnMatch(k = 2) + Lowe's ratio  (reference src/Frame.cc:1231-1255)
//   k_fisheye_triangulate, k_fisheye_triangulate_batch  the triangulation filter                  (src/Frame.cc:1256-1271, kb8_triangulate.h)
//   k_lap_gather_batch                                  the reference's keypoint order            (src/ORBextractor.cc:1466-1487)
//   k_hamming_pairs                                     ORBmatcher::DescriptorDistance            (src/ORBmatcher.cc:2256-2272): eight lines
//                                                       of the same brute-force Hamming family, filed here for want of a family of its own
// The batched three run one behind the other on the job records of a batch (ft_tracked_batch_bind_fisheye, tracked_batch.cpp).
// Host side of the one-frame calls: fisheye_match.cpp.
#include "ft_internal.h"
#include "ft_search.h"
#include "kb8_triangulate.h"
#include "wave_ops.h"

namespace {

// Brute-force 2-NN: one wave per query, lanes stride over the train set; the two smallest
// (distance, index) keys of the wave are the reference's (best, second) with earlier index first.
__global__ __launch_bounds__(256) void k_fisheye_2nn(const uint8_t *descL, int nL, const uint8_t *descR, int nR,
                                                     int *matches, int *bestOut, int *secondOut) {
    const int lane = threadIdx.x & 63, wave = wave_index();
    const int i = blockIdx.x * 4 + wave;
    if (i >= nL) return;
    unsigned long long q[4];
    {
        const unsigned long long *p = (const unsigned long long *)(descL + (size_t)i * 32);
        q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = p[3];
    }
    unsigned k0 = 0xffffffffu, k1 = 0xffffffffu;  // two smallest keys seen by this lane
    for (int j = lane; j < nR; j += 64) {
        const unsigned key = ((unsigned)hamming256(q, (const unsigned long long *)(descR + (size_t)j * 32)) << 20) | (unsigned)j;
        if (key < k0) { k1 = k0; k0 = key; }
        else if (key < k1) k1 = key;
    }
    const unsigned m0 = wave_min_u32(k0);
    // second smallest overall: lanes whose k0 was the global minimum contribute their k1 instead
    const unsigned cand = (k0 == m0) ? k1 : k0;
    const unsigned m1 = wave_min_u32(cand);
    if (lane == 0) {
        const int d0 = (int)(m0 >> 20), d1 = (int)(m1 >> 20);
        int match = -1;
        if (nR >= 2 && (double)(float)d0 < (double)(float)d1 * 0.7) match = (int)(m0 & 0xfffffu);
        matches[i] = match;
        if (bestOut) bestOut[i] = nR >= 1 ? d0 : -1;
        if (secondOut) secondOut[i] = nR >= 2 ? d1 : -1;
    }
}

__global__ __launch_bounds__(256) void k_hamming_pairs(const uint8_t *a, const uint8_t *b, int n, int *dist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long *pa = (const unsigned long long *)(a + (size_t)i * 32);
    unsigned long long q[4] = {pa[0], pa[1], pa[2], pa[3]};
    dist[i] = hamming256(q, (const unsigned long long *)(b + (size_t)i * 32));
}

// KannalaBrandt8::TriangulateMatches (kb8_triangulate.h) for the pairs that passed the ratio test: one thread per left keypoint.
__global__ __launch_bounds__(64) void k_fisheye_triangulate(FtFisheyeRig rig, const ft_keypoint *keysL, int nL, const ft_keypoint *keysR,
                                                           int *matches, float *depth, float *p3d, int *nMatches) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= nL) return;
    const int j = matches[i];
    float d = -1.0f, p[3] = {0.f, 0.f, 0.f};
    int m = -1;
    if (j >= 0) {
        const ft_keypoint a = keysL[i], b = keysR[j];
        const float z = kb8_triangulate_matches(rig.cam1, rig.cam2, rig.precision, rig.Rlr, rig.tlr, a.x, a.y, b.x, b.y, rig.sigma2[a.octave], rig.sigma2[b.octave], p);
        if (z > 0.0001f) {  // Frame.cc:1263
            d = z;
            m = j;
            atomicAdd(nMatches, 1);
        } else {
            p[0] = p[1] = p[2] = 0.f;
        }
    }
    matches[i] = m;
    depth[i] = d;
    p3d[3 * i] = p[0];
    p3d[3 * i + 1] = p[1];
    p3d[3 * i + 2] = p[2];
}

// ---- two-camera frames of a batch straight from what two extractors left in HBM (ft_tracked_batch_bind_fisheye) ----
// Step 1, workgroup (camera, frame): the keypoints and descriptors of the extractor's slot into the frame's arrays in the
// REFERENCE's order - ORBextractor::operator() fills keypoints inside the lapping area from the back and the others from the
// front (src/ORBextractor.cc:1466-1487; assembleOutputs, extractor.cpp, does the same for the host copies) - a stable
// partition by ranks from ballots; also: the camera's match table = -1, and the number of keypoints outside the lapping
// area (monoLeft / monoRight, src/Frame.cc:1144-1147) for step 2.
__global__ __launch_bounds__(256) void k_lap_gather_batch(const FtBatchJob *__restrict__ jobs, Rebase rb, FtBindArgs A) {
    const int cam = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FtDevFrame &F = jobs[f].F;
    const int slot = (cam == 0 ? A.slot0L : A.slot0R) + f;
    const int n = cam == 0 ? F.Nleft : F.N - F.Nleft;
    const ft_keypoint *src = (cam == 0 ? A.keysL : A.keysR) + (size_t)slot * (cam == 0 ? A.strideL : A.strideR);
    const uint4 *srcD = (const uint4 *)((cam == 0 ? A.descL : A.descR) + (size_t)slot * (cam == 0 ? A.strideL : A.strideR) * 32);
    ft_keypoint *dst = (ft_keypoint *)rb(cam == 0 ? F.keys : F.keysR);
    uint4 *dstD = (uint4 *)(rb((uint8_t *)F.desc) + (cam == 0 ? 0 : (size_t)F.Nleft * 32));
    int *tab = (int *)rb(cam == 0 ? F.l2r : F.r2l);
    const float lap0 = (float)(cam == 0 ? A.lapL0 : A.lapR0), lap1 = (float)(cam == 0 ? A.lapL1 : A.lapR1);
    __shared__ int wLap[4];
    int lapBefore = 0;  // lapping-area keypoints in front of this chunk
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        ft_keypoint kp;
        bool inLap = false;
        if (i < n) {
            kp = src[i];
            inLap = kp.x >= lap0 && kp.x <= lap1;
        }
        const unsigned long long b = __ballot(inLap);
        if (lane == 0) wLap[wave] = __popcll(b);
        __syncthreads();
        int before = lapBefore;
        for (int w = 0; w < wave; w++) before += wLap[w];
        const int chunkLap = wLap[0] + wLap[1] + wLap[2] + wLap[3];
        __syncthreads();
        if (i < n) {
            const int rankLap = before + __popcll(b & ((1ull << lane) - 1ull));
            const int d = inLap ? n - 1 - rankLap : i - rankLap;
            dst[d] = kp;
            dstD[2 * (size_t)d] = srcD[2 * (size_t)i];
            dstD[2 * (size_t)d + 1] = srcD[2 * (size_t)i + 1];
            tab[i] = -1;
        }
        lapBefore += chunkLap;
    }
    if (tid == 0) {
        A.mono[2 * f + cam] = n - lapBefore;
        if (cam == 0 && A.nMatches) A.nMatches[f] = 0;
    }
}

// Step 2: the matching part of Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1231-1255; the seam of the reference's
// launchFisheyeStereoMatchKernel, include/Kernels/KernelController.h:38) for every frame of the batch: BFMatcher(NORM_HAMMING)
// .knnMatch(k = 2) of the left lapping subset [monoLeft, Nleft) against the right one + Lowe's ratio 0.7, written as
// mvLeftToRightMatch / mvRightToLeftMatch (a right keypoint matched by several left ones keeps the last = largest index, as the
// reference's loop does).  A wave takes FE_Q queries: a lane holds one train descriptor of the current 64 in registers and
// meets the queries through LDS broadcasts, so a train descriptor is fetched once per FE_Q queries (the one-query-per-wave
// form of k_fisheye_2nn reads the whole train set per query: 128 MB of L2 traffic per 2000 x 2000 frame); keys
// (distance << 20 | train index), two smallest per lane and query, one wave reduction per query at the end.
#define FE_Q 16
// fillR2l = 0: the triangulation filter follows (k_fisheye_triangulate_batch), which writes mvRightToLeftMatch for the pairs it keeps
__global__ __launch_bounds__(256) void k_fisheye_2nn_batch(const FtBatchJob *__restrict__ jobs, Rebase rb, const int *__restrict__ mono,
                                                           int fillR2l) {
    const int f = blockIdx.y, lane = threadIdx.x & 63, wave = wave_index();
    const FtDevFrame &F = jobs[f].F;
    const int monoL = mono[2 * f], monoR = mono[2 * f + 1];
    const int nQ = F.Nleft - monoL, nT = (F.N - F.Nleft) - monoR;
    const int q0 = (blockIdx.x * 4 + wave) * FE_Q;
    if (q0 >= nQ) return;
    const uint8_t *desc = rb(F.desc);
    const uint4 *qd = (const uint4 *)(desc + (size_t)(monoL + q0) * 32);
    const uint4 *td = (const uint4 *)(desc + (size_t)(F.Nleft + monoR) * 32);
    __shared__ uint4 qs[4][FE_Q * 2];
    const int nq = min(FE_Q, nQ - q0);
    if (lane < 2 * nq) qs[wave][lane] = qd[lane];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    unsigned k0[FE_Q], k1[FE_Q];
#pragma unroll
    for (int q = 0; q < FE_Q; q++) k0[q] = k1[q] = 0xffffffffu;
    // (the next train descriptor is requested before the current one is compared with the sixteen queries: 320 vector
    // instructions cover its round trip, where two waves per SIMD - 175 registers - could not)
    uint4 an = make_uint4(0, 0, 0, 0), bn = an;
    if (lane < nT) {
        an = td[2 * (size_t)lane];
        bn = td[2 * (size_t)lane + 1];
    }
    for (int j = lane; j < nT; j += 64) {
        const uint4 a = an, b = bn;
        if (j + 64 < nT) {
            an = td[2 * (size_t)(j + 64)];
            bn = td[2 * (size_t)(j + 64) + 1];
        }
#pragma unroll
        for (int q = 0; q < FE_Q; q++) {
            const uint4 x = qs[wave][2 * q], y = qs[wave][2 * q + 1];  // (same address in every lane: a broadcast)
            const unsigned d = __popc(a.x ^ x.x) + __popc(a.y ^ x.y) + __popc(a.z ^ x.z) + __popc(a.w ^ x.w) + __popc(b.x ^ y.x) +
                               __popc(b.y ^ y.y) + __popc(b.z ^ y.z) + __popc(b.w ^ y.w);
            const unsigned key = (d << 20) | (unsigned)j;
            k1[q] = min(k1[q], max(k0[q], key));
            k0[q] = min(k0[q], key);
        }
    }
    int *l2r = (int *)rb(F.l2r), *r2l = (int *)rb(F.r2l);
#pragma unroll
    for (int q = 0; q < FE_Q; q++) {
        const unsigned m0 = wave_min_u32(k0[q]);
        const unsigned cand = (k0[q] == m0) ? k1[q] : k0[q];
        const unsigned m1 = wave_min_u32(cand);
        if (lane == 0 && q < nq) {
            const int d0 = (int)(m0 >> 20), d1 = (int)(m1 >> 20);
            if (nT >= 2 && (double)(float)d0 < (double)(float)d1 * 0.7) {
                const int t = monoR + (int)(m0 & 0xfffffu), qi = monoL + q0 + q;
                l2r[qi] = t;
                if (fillR2l) atomicMax(&r2l[t], qi);
            }
        }
    }
}

// Step 3, k_fisheye_triangulate for every frame of the batch (blockIdx.y = frame): the pairs k_fisheye_2nn_batch left in mvLeftToRightMatch
// (right-camera indices) are triangulated; a pair that fails loses its entry, a pair that stays enters mvRightToLeftMatch (the
// largest left index per right keypoint = the last writer of the reference's loop, src/Frame.cc:1262) and mvDepth / mvStereo3Dpoints
__global__ __launch_bounds__(256) void k_fisheye_triangulate_batch(const FtBatchJob *__restrict__ jobs, Rebase rb, FtBindArgs A) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const FtDevFrame &F = jobs[f].F;
    if (i >= F.Nleft) return;
    int *l2r = (int *)rb(F.l2r), *r2l = (int *)rb(F.r2l);
    const int j = l2r[i];
    float d = -1.0f, p[3] = {0.f, 0.f, 0.f};
    if (j >= 0) {
        const ft_keypoint a = rb(F.keys)[i], b = rb(F.keysR)[j];
        const float z = kb8_triangulate_matches(A.rig.cam1, A.rig.cam2, A.rig.precision, A.rig.Rlr, A.rig.tlr, a.x, a.y, b.x, b.y, A.rig.sigma2[a.octave], A.rig.sigma2[b.octave], p);
        if (z > 0.0001f) {  // Frame.cc:1263
            d = z;
            atomicMax(&r2l[j], i);
            atomicAdd(&A.nMatches[f], 1);
        } else {
            p[0] = p[1] = p[2] = 0.f;
            l2r[i] = -1;
        }
    }
    if (A.depth) {
        float *dep = rb(A.depth[f]), *pp = rb(A.p3d[f]);
        dep[i] = d;
        pp[3 * i] = p[0];
        pp[3 * i + 1] = p[1];
        pp[3 * i + 2] = p[2];
    }
}

}  // namespace

int ft_launch_fisheye(hipStream_t st, const uint8_t *descL, int nL, const uint8_t *descR, int nR, int *matches,
                      int *best, int *second) {
    if (nL <= 0) return FT_OK;
    hipLaunchKernelGGL(k_fisheye_2nn, dim3((nL + 3) / 4), dim3(256), 0, st, descL, nL, descR, nR, matches, best, second);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_fisheye_triangulate(hipStream_t st, const FtFisheyeRig &rig, const ft_keypoint *keysL, int nL,
                                  const ft_keypoint *keysR, int *matches, float *depth, float *p3d, int *nMatches) {
    if (nL <= 0) return FT_OK;
    hipLaunchKernelGGL(k_fisheye_triangulate, dim3((nL + 63) / 64), dim3(64), 0, st, rig, keysL, nL, keysR, matches, depth, p3d, nMatches);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_hamming_pairs(hipStream_t st, const uint8_t *a, const uint8_t *b, int n, int *dist) {
    if (n <= 0) return FT_OK;
    hipLaunchKernelGGL(k_hamming_pairs, dim3((n + 255) / 256), dim3(256), 0, st, a, b, n, dist);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

// ---- launches of a batch of frames (ft_tracked_batch_bind_fisheye, tracked_batch.cpp) ----
int ft_launch_bind_fisheye_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxKp, const FtBindArgs &A) {
    if (nFrames <= 0) return FT_OK;
    hipLaunchKernelGGL(k_lap_gather_batch, dim3(2, nFrames), dim3(256), 0, st, jobs, rebase_of(arena), A);
    hipLaunchKernelGGL(k_fisheye_2nn_batch, dim3((maxKp + 4 * FE_Q - 1) / (4 * FE_Q), nFrames), dim3(256), 0, st, jobs, rebase_of(arena),
                       (const int *)A.mono, A.triangulate ? 0 : 1);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_fisheye_triangulate_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxKp, const FtBindArgs &A) {
    if (nFrames <= 0 || maxKp <= 0) return FT_OK;
    hipLaunchKernelGGL(k_fisheye_triangulate_batch, dim3((maxKp + 255) / 256, nFrames), dim3(256), 0, st, jobs, rebase_of(arena), A);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

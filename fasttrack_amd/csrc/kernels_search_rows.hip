// HIP kernels of the projection searches for the frames of a batch (ft_tracked_batch) in which a map point is a ROW of 16
// lanes, four points per wave - EXPERIMENTS.md sections 10 and 11 (the lean later passes; the first pass, the window scan
// through a row's LDS list, the partition of the candidate lists):
//   k_search_last_first, k_search_local_first   the first pass of the claim iteration: window scans that file the candidate lists
//   k_cache_partition_batch                     behind it: the best candidates of every list to its front
//   k_search_last_lean, k_search_local_lean     a later pass served from the lists; what they cannot serve goes to the slow list
// They compute what the wave-per-point kernels compute (kernels_search.hip: ORBmatcher::SearchByProjection, reference
// src/ORBmatcher.cc:49-225 and :1775-1960) and file what those file, so a search may mix the two forms pass by pass.
#include <algorithm>

#include "search_dev.h"

namespace {

// ---- first pass of a batch, four points per wave --------------------------------------------------------------------------
// The general kernel (kernels_search.hip) gives the window scan of ONE point a whole wave: at th 7 a window holds ~50 candidates of a few (octave,
// column) ranges - most lanes idle through ~600 instructions per point.  Here a point is a ROW of 16 lanes from the start
// (as in the lean kernels of the later passes): the ranges of its window one per lane (a DPP scan inside the row lays them end
// to end), the entries 16 at a time (the range of an entry by a few row-local shuffles), the candidates filed in the point's
// cache at positions handed out by a ballot of the row (no LDS counter), the minimum (two minima) by DPP steps inside the row.
// What is computed per entry - box, level band, uright test, Hamming distance, key - and what is filed are exactly the
// general kernel's (the order of a list is free), so the later passes cannot tell which kernel ran the first one.  First pass:
// nothing is locked but what was held before the call.
// the two smallest keys of a row, in every lane of it
__device__ __forceinline__ void row_two_min(unsigned long long &k0, unsigned long long &k1) {
    const unsigned long long m0 = row_min_u64(k0);
    const unsigned long long cand = (k0 == m0) ? k1 : k0;
    k1 = row_min_u64(cand);
    k0 = m0;
}

// (row_for_window, the window scan of a row's point through its LDS list: search_dev.h - the Fuse search of kernels_fuse.hip shares it)
// a candidate key into the point's list: positions by a ballot of the row (n = candidates filed so far, row-uniform)
__device__ __forceinline__ void row_cache_append(unsigned long long *slot, int &n, bool cand, unsigned long long key, int sub, int rowBase) {
    const unsigned bits = (unsigned)(__ballot(cand) >> rowBase) & 0xffffu;
    if (cand) {
        const int pos = n + __popc(bits & ((1u << sub) - 1u));
        if (pos < FT_CACHE_CAP) slot[1 + pos] = key;
    }
    n += __popc(bits);
}
__device__ __forceinline__ void row_cache_end(unsigned long long *slot, int n, bool anyInBox, int sub) {
    if (sub == 0)
        slot[0] = (unsigned long long)(unsigned)n | ((unsigned long long)(anyInBox ? 1 : 0) << 32) | ((unsigned long long)(unsigned)min(n, FT_CACHE_CAP) << 40);
}
__device__ __forceinline__ bool row_any(bool v, int rowBase) { return ((unsigned)(__ballot(v) >> rowBase) & 0xffffu) != 0u; }
// the first pass's claims_file for the point of a row: no previous results, every result counts as changed (the flag was set by
// claims_begin_pass)
__device__ __forceinline__ void claims_file_row_first(const FtClaims &C, int *res, int i, int sub, const int r4[4]) {
    if (sub < 4) {
        const int kp = sub == 0 ? r4[0] : sub == 1 ? r4[1] : sub == 2 ? r4[2] : r4[3];
        const int s = 4 * i + sub;
        res[s] = kp;
        if (kp >= 0) {
            const int e = (s << 1) | (C.obs[i] > 0 ? 1 : 0);
            int *rec = C.tabWrite + 8 * (size_t)kp;
            const int pos = atomicAdd(rec, 1) + 1;
            if (pos < FT_TAB_ENTRIES) rec[1 + pos] = e;
            else C.nextWrite[s] = atomicExch(&C.headWrite[kp], e);
        }
    }
}

__global__ __launch_bounds__(256) void k_search_last_first(const FtBatchJob *__restrict__ jobs, Rebase rb, float th, FtSlotGrid sg) {
    int frame, blk;
    if (!ft_slot_block(sg, frame, blk)) return;
    const FtBatchJob &J = jobs[frame];
    if (J.nPoints <= 0) return;
    int *res;
    const FtClaims C = job_claims(J, rb, 0, 0, -1, FT_BATCH_FLAGS / 2, res);
    claims_begin_pass(C, blk, sg.blocksPerSlot);
    __shared__ unsigned rowLists[16][FT_ROW_LIST];
    unsigned *list = rowLists[threadIdx.x >> 4];
    const int lane = threadIdx.x & 63, sub = lane & 15, rowBase = lane & 48;
    const int i = blk * 16 + (threadIdx.x >> 4);
    if (i >= J.L.N) return;
    const FtDevFrame &F = J.F;
    const FramePtrs Q = frame_ptrs(F, rb);
    const bool twoCam = F.Nleft != -1;
    unsigned long long *slotL = C.cache + (size_t)i * FT_CACHE_WORDS, *slotR = slotL + (FT_CACHE_CAP + 1);
    int primL = -1, primR = -1;
    if (rb(J.L.valid)[i]) {
        const FtLastProj pj = rb(J.proj)[i];
        if (!pj.go) {
            if (sub == 0) slotL[0] = 0ull;  // does not project into the image: an empty list spares the later passes the question
        } else {
            const int oct = rb(J.L.octave)[i];
            const float radius = __fmul_rn(th, F.sf[oct]);
            int minLevel, maxLevel;
            if (J.forward) { minLevel = oct; maxLevel = -1; }
            else if (J.backward) { minLevel = 0; maxLevel = oct; }
            else { minLevel = oct - 1; maxLevel = oct + 1; }
            unsigned long long q[4];
            {
                const unsigned long long *p = (const unsigned long long *)(rb(J.L.desc) + (size_t)i * 32);
                q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = p[3];
            }
            const float u = pj.u, v = pj.v;
            const Window w = cell_window(F, u, v, radius);
            unsigned long long k0 = KEY_NONE;
            int n = 0;
            bool anyCand = false;
            if (!w.empty) {
                row_for_window(F, Q, 0, w, minLevel, maxLevel, u, v, radius, sub, rowBase, list, [&](const WinEntry &kp, bool real) {
                    const bool inb = real;  // (in_box held in the filter step)
                    anyCand = anyCand || inb;
                    bool cand = inb;
                    if (cand && kp.uright > 0) {
                        const float ur = __fsub_rn(u, __fmul_rn(F.mbf, pj.invzc));
                        if (fabsf(__fsub_rn(ur, kp.uright)) > radius) cand = false;
                    }
                    const bool held = cand && Q.holderObs[cand ? kp.idx : 0] > 0;
                    const unsigned long long key = make_key(hamming256(q, kp.d), kp.cx, kp.cy, kp.idx, kp.octave, held);
                    row_cache_append(slotL, n, cand, key, sub, rowBase);
                    if (cand && !held) k0 = key < k0 ? key : k0;
                });
            }
            anyCand = row_any(anyCand, rowBase);
            row_cache_end(slotL, n, anyCand, sub);
            k0 = row_min_u64(k0);
            if (anyCand) {  // `if(vIndices2.empty()) continue;` (ORBmatcher.cc:1836) also skips the right-camera block
                if (k0 != KEY_NONE && key_dist(k0) <= FT_TH_HIGH) primL = key_idx(k0);
                if (twoCam) {
                    const float ur = pj.ur, vr = pj.vr;
                    const Window wr = cell_window(F, ur, vr, radius);
                    unsigned long long kr = KEY_NONE;
                    int nr = 0;
                    if (!wr.empty) {
                        row_for_window(F, Q, 1, wr, minLevel, maxLevel, ur, vr, radius, sub, rowBase, list, [&](const WinEntry &kp, bool real) {
                            const bool cand = real;
                            const bool held = cand && Q.holderObs[(cand ? kp.idx : 0) + F.Nleft] > 0;
                            const unsigned long long key = make_key(hamming256(q, kp.d), kp.cx, kp.cy, kp.idx, kp.octave, held);
                            row_cache_append(slotR, nr, cand, key, sub, rowBase);
                            if (cand && !held) kr = key < kr ? key : kr;
                        });
                    }
                    row_cache_end(slotR, nr, false, sub);
                    kr = row_min_u64(kr);
                    if (kr != KEY_NONE && key_dist(kr) <= FT_TH_HIGH) primR = key_idx(kr) + F.Nleft;
                }
            }
        }
    }
    const int r4[4] = {primL, -1, primR, -1};
    claims_file_row_first(C, res, i, sub, r4);
}

__global__ __launch_bounds__(256) void k_search_local_first(const FtBatchJob *__restrict__ jobs, Rebase rb, float th, float nnRatio, FtSlotGrid sg) {
    int frame, blk;
    if (!ft_slot_block(sg, frame, blk)) return;
    const FtBatchJob &J = jobs[frame];
    if (J.nPoints <= 0) return;
    int *res;
    const FtClaims C = job_claims(J, rb, 0, 0, -1, FT_BATCH_FLAGS / 2, res);
    claims_begin_pass(C, blk, sg.blocksPerSlot);
    __shared__ unsigned rowLists[16][FT_ROW_LIST];
    unsigned *list = rowLists[threadIdx.x >> 4];
    const int lane = threadIdx.x & 63, sub = lane & 15, rowBase = lane & 48;
    const int i = blk * 16 + (threadIdx.x >> 4);
    if (i >= J.P.M) return;
    const FtDevFrame &F = J.F;
    const FramePtrs Q = frame_ptrs(F, rb);
    const bool twoCam = F.Nleft != -1;
    unsigned long long *slotL = C.cache + (size_t)i * FT_CACHE_WORDS, *slotR = slotL + (FT_CACHE_CAP + 1);
    const uint8_t skipV = rb(J.P.skip)[i], inViewV = rb(J.P.inView)[i], inViewRV = twoCam ? rb(J.P.inViewR)[i] : (uint8_t)0;
    const int levelRV = twoCam ? rb(J.P.levelR)[i] : -1;
    const int obsI = C.obs[i];
    int primL = -1, sideL = -1, primR = -1, sideR = -1;
    bool skipRight = false;
    if (!skipV) {
        unsigned long long q[4];
        {
            const unsigned long long *p = (const unsigned long long *)(rb(J.P.desc) + (size_t)i * 32);
            q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = p[3];
        }
        if (inViewV) {
            const int level = rb(J.P.level)[i];
            float r = ((double)rb(J.P.viewCos)[i] > 0.998) ? 2.5f : 4.0f;  // RadiusByViewingCos, ORBmatcher.cc:314-320
            if ((double)th != 1.0) r = __fmul_rn(r, th);
            const float rad = __fmul_rn(r, F.sf[level]);
            const float x = rb(J.P.projX)[i], y = rb(J.P.projY)[i];
            const Window w = cell_window(F, x, y, rad);
            unsigned long long k0 = KEY_NONE, k1 = KEY_NONE;
            int n = 0;
            if (!w.empty) {
                const float pxr = (F.Nleft == -1 && Q.uright) ? rb(J.P.projXR)[i] : 0.f;
                row_for_window(F, Q, 0, w, level - 1, level, x, y, rad, sub, rowBase, list, [&](const WinEntry &kp, bool real) {
                    bool cand = real;
                    if (cand && kp.uright > 0 && fabsf(__fsub_rn(pxr, kp.uright)) > rad) cand = false;  // (mono-stereo frames only)
                    const bool held = cand && Q.holderObs[cand ? kp.idx : 0] > 0;
                    const unsigned long long key = make_key(hamming256(q, kp.d), kp.cx, kp.cy, kp.idx, kp.octave, held);
                    row_cache_append(slotL, n, cand, key, sub, rowBase);
                    if (cand && !held) two_min_insert(k0, k1, key);
                });
            }
            row_cache_end(slotL, n, false, sub);
            row_two_min(k0, k1);
            int bd = 256, bd2 = 256, bl = -1, bl2 = -1, bi = -1;
            if (k0 != KEY_NONE) { bd = key_dist(k0); bi = key_idx(k0); bl = key_octave(k0); }
            if (k1 != KEY_NONE) { bd2 = key_dist(k1); bl2 = key_octave(k1); }
            if (bd <= FT_TH_HIGH) {
                if (bl == bl2 && (float)bd > __fmul_rn(nnRatio, (float)bd2)) skipRight = true;
                else {
                    primL = bi;
                    if (twoCam) {
                        const int m = Q.l2r[bi];
                        if (m != -1) sideL = m + F.Nleft;
                    }
                }
            }
        }
        // (a point whose left block ended in the ratio test's `continue` files its right-camera candidates all the same: a later
        // pass may get past the test - the locks decide - and would otherwise have to come back here through the slow list)
        if (twoCam && inViewRV && levelRV != -1) {
            const int level = levelRV;
            const float r = ((double)rb(J.P.viewCosR)[i] > 0.998) ? 2.5f : 4.0f;
            const float rad = __fmul_rn(r, F.sf[level]);
            const float x = rb(J.P.projXR)[i], y = rb(J.P.projYR)[i];
            const Window w = cell_window(F, x, y, rad);
            unsigned long long k0 = KEY_NONE, k1 = KEY_NONE;
            int n = 0;
            if (!w.empty) {
                row_for_window(F, Q, 1, w, level - 1, level, x, y, rad, sub, rowBase, list, [&](const WinEntry &kp, bool real) {
                    const bool cand = real;
                    const int g = kp.idx + F.Nleft;
                    const bool held = cand && Q.holderObs[cand ? g : 0] > 0;
                    // this point's own left-block side write precedes its right-block search
                    const bool locked = (g == sideL) ? (obsI > 0) : held;
                    const unsigned long long key = make_key(hamming256(q, kp.d), kp.cx, kp.cy, kp.idx, kp.octave, held);
                    row_cache_append(slotR, n, cand, key, sub, rowBase);
                    if (cand && !locked) two_min_insert(k0, k1, key);
                });
            }
            row_cache_end(slotR, n, false, sub);
            row_two_min(k0, k1);
            int bdr = 256, bd2r = 256, blr = -1, bl2r = -1, bir = -1;
            if (k0 != KEY_NONE) { bdr = key_dist(k0); bir = key_idx(k0); blr = key_octave(k0); }
            if (k1 != KEY_NONE) { bd2r = key_dist(k1); bl2r = key_octave(k1); }
            if (!skipRight && bdr <= FT_TH_HIGH && !(blr == bl2r && (float)bdr > __fmul_rn(nnRatio, (float)bd2r))) {
                const int m = Q.r2l[bir];
                if (m != -1) sideR = m;
                primR = bir + F.Nleft;
            }
        }
    }
    const int r4[4] = {primL, sideL, primR, sideR};
    claims_file_row_first(C, res, i, sub, r4);
}

// ---- later passes of a batch: the lean kernels --------------------------------------------------------------------------------
// From the second pass on nearly every point finds its candidates in the cache the first pass filed, and its turn is a
// handful of loads: the cached keys, the 32-byte writer records of their keypoints, a minimum.  The general kernels (kernels_search.hip)
// spend a whole wave (and ~90 registers, 30 KB of code) on it.  Here a point is a ROW of 16 lanes - four points per wave, the
// keys 16 at a time, the two smallest by DPP steps that never leave the row - and a point the cache cannot serve (a camera's
// candidates not filed yet: the right block is reached for the first time; more candidates than the cache holds) is handed
// to the general kernel through the frame's slow list (launched behind this one with slowList = 1).  Same reads of the
// previous pass's records, same keys, same comparisons: the results are those of the general kernel.
// claims_file for the point of a row: lane `sub` (0 .. 3) of the row files write kind sub
__device__ __forceinline__ void claims_file_row(const FtClaims &C, int *res, int i, int sub, const int r4[4]) {
    if (sub < 4) {
        const int kp = sub == 0 ? r4[0] : sub == 1 ? r4[1] : sub == 2 ? r4[2] : r4[3];
        const int s = 4 * i + sub;
        const int prev = shared_load(&C.resPrev[s]);
        if (kp != prev) atomicAnd(C.flagCur, 0);
        shared_store(&res[s], kp);
        if (kp >= 0) {
            const int e = (s << 1) | (C.obs[i] > 0 ? 1 : 0);
            int *rec = C.tabWrite + 8 * (size_t)kp;
            const int pos = atomicAdd(rec, 1) + 1;
            if (pos < FT_TAB_ENTRIES) shared_store(rec + 1 + pos, e);
            else shared_store(&C.nextWrite[s], atomicExch(&C.headWrite[kp], e));
        }
    }
}
__device__ __forceinline__ void slow_append(int *slow, int pass, int nPoints, int i) {
    const int pos = atomicAdd(&slow[pass & 1], 1);
    slow[16 + (size_t)(pass & 1) * nPoints + pos] = i;
}
#define FT_LEAN_PPB 16  // points per workgroup of the lean kernels: 4 waves x 4 rows

__global__ __launch_bounds__(256) void k_search_local_lean(const FtBatchJob *__restrict__ jobs, Rebase rb, int pass, int fCur, int fPrev,
                                                           int fReset, float nnRatio) {
    const FtBatchJob &J = jobs[blockIdx.y];
    if (J.nPoints <= 0) return;
    int *res;
    const FtClaims C = job_claims(J, rb, pass, fCur, fPrev, fReset, res);
    if (!claims_begin_pass(C)) return;
    int *slow = rb(J.slow);
    if (blockIdx.x == 0 && threadIdx.x == 0) slow[(pass + 1) & 1] = 0;  // the next pass's list starts empty
    const int sub = threadIdx.x & 15;
    const int i = blockIdx.x * FT_LEAN_PPB + (threadIdx.x >> 4);
    if (i >= J.P.M) return;
    const FtDevFrame &F = J.F;
    const bool twoCam = F.Nleft != -1;
    const uint8_t *skipP = rb(J.P.skip), *inViewP = rb(J.P.inView), *inViewRP = rb(J.P.inViewR);
    const int *levelRP = rb(J.P.levelR);
    const unsigned long long *slotL = C.cache + (size_t)i * FT_CACHE_WORDS, *slotR = slotL + (FT_CACHE_CAP + 1);
    const uint8_t skipV = skipP[i], inViewV = inViewP[i], inViewRV = twoCam ? inViewRP[i] : (uint8_t)0;
    const int levelRV = twoCam ? levelRP[i] : -1;
    const unsigned long long metaL = slotL[0], metaR = twoCam ? slotR[0] : KEY_NONE;
    const int obsI = C.obs[i];
    // A pass is a chain of dependent round trips, and the chip is full of such chains: the first 16 keys of both cameras'
    // lists are requested together with the flags and the meta words, and the lock records of both - the right camera's on
    // the chance that its block is reached - in ONE further trip (flags -> meta -> keys -> records left -> l2r -> records right
    // used to be six).  A key beyond a list's head is not a key: its "record" is the one of keypoint 0, read and dropped.
    const unsigned long long keyL0 = slotL[1 + sub], keyR0 = twoCam ? slotR[1 + sub] : KEY_NONE;
    const int headL0 = metaL == KEY_NONE ? 0 : min(cache_head(metaL), FT_CACHE_CAP), headR0 = metaR == KEY_NONE ? 0 : min(cache_head(metaR), FT_CACHE_CAP);
    const bool haveL0 = sub < headL0, haveR0 = sub < headR0;
    const int kpL0 = haveL0 ? key_idx(keyL0) : 0, kpR0 = haveR0 ? key_idx(keyR0) + F.Nleft : 0;
    const LockRec recL0 = lock_record(C, kpL0), recR0 = lock_record(C, kpR0);
    int primL = -1, sideL = -1, primR = -1, sideR = -1;
    bool skipRight = false, slowPoint = false;
    if (!skipV) {
        if (inViewV) {
            int nCached;
            bool anyBox;
            if (cache_state_of(metaL, nCached, anyBox) != 1) slowPoint = true;
            else {
                unsigned long long k0 = KEY_NONE, k1 = KEY_NONE;
                const int head = cache_head(metaL);
                if (haveL0 && !locked_by(C, recL0, kpL0, i, key_held(keyL0))) k0 = keyL0;
                for (int t = 16 + sub; t < head; t += 16) {
                    const unsigned long long key = slotL[1 + t];
                    if (is_locked(C, key_idx(key), i, key_held(key))) continue;
                    two_min_insert(k0, k1, key);
                }
                row_two_min(k0, k1);
                if (k1 == KEY_NONE && head < nCached) {  // fewer than two unlocked keys in the head: the rest of the list decides
                    for (int t = head + sub; t < nCached; t += 16) {
                        const unsigned long long key = slotL[1 + t];
                        if (is_locked(C, key_idx(key), i, key_held(key))) continue;
                        two_min_insert(k0, k1, key);
                    }
                    row_two_min(k0, k1);
                }
                int bd = 256, bd2 = 256, bl = -1, bl2 = -1, bi = -1;
                if (k0 != KEY_NONE) { bd = key_dist(k0); bi = key_idx(k0); bl = key_octave(k0); }
                if (k1 != KEY_NONE) { bd2 = key_dist(k1); bl2 = key_octave(k1); }
                if (bd <= FT_TH_HIGH) {
                    if (bl == bl2 && (float)bd > __fmul_rn(nnRatio, (float)bd2)) skipRight = true;
                    else {
                        primL = bi;
                        if (twoCam) {
                            const int m = rb(F.l2r)[bi];
                            if (m != -1) sideL = m + F.Nleft;
                        }
                    }
                }
            }
        }
        if (!slowPoint && twoCam && inViewRV && !skipRight && levelRV != -1) {
            int nCached;
            bool anyBox;
            if (cache_state_of(metaR, nCached, anyBox) != 1) slowPoint = true;
            else {
                unsigned long long k0 = KEY_NONE, k1 = KEY_NONE;
                const int head = cache_head(metaR);
                auto scan = [&](int from, int to) {
                    for (int t = from + sub; t < to; t += 16) {
                        const unsigned long long key = slotR[1 + t];
                        const int g = key_idx(key) + F.Nleft;
                        const bool locked = (g == sideL) ? (obsI > 0) : is_locked(C, g, i, key_held(key));
                        if (locked) continue;
                        two_min_insert(k0, k1, key);
                    }
                    row_two_min(k0, k1);
                };
                if (haveR0 && !((kpR0 == sideL) ? (obsI > 0) : locked_by(C, recR0, kpR0, i, key_held(keyR0)))) k0 = keyR0;
                scan(16, head);
                if (k1 == KEY_NONE && head < nCached) scan(head, nCached);
                int bdr = 256, bd2r = 256, blr = -1, bl2r = -1, bir = -1;
                if (k0 != KEY_NONE) { bdr = key_dist(k0); bir = key_idx(k0); blr = key_octave(k0); }
                if (k1 != KEY_NONE) { bd2r = key_dist(k1); bl2r = key_octave(k1); }
                if (bdr <= FT_TH_HIGH && !(blr == bl2r && (float)bdr > __fmul_rn(nnRatio, (float)bd2r))) {
                    const int m = rb(F.r2l)[bir];
                    if (m != -1) sideR = m;
                    primR = bir + F.Nleft;
                }
            }
        }
    }
    if (slowPoint) {
        if (sub == 0) slow_append(slow, pass, J.nPoints, i);
        return;
    }
    const int r4[4] = {primL, sideL, primR, sideR};
    claims_file_row(C, res, i, sub, r4);
}

__global__ __launch_bounds__(256) void k_search_last_lean(const FtBatchJob *__restrict__ jobs, Rebase rb, int pass, int fCur, int fPrev,
                                                          int fReset) {
    const FtBatchJob &J = jobs[blockIdx.y];
    if (J.nPoints <= 0) return;
    int *res;
    const FtClaims C = job_claims(J, rb, pass, fCur, fPrev, fReset, res);
    if (!claims_begin_pass(C)) return;
    int *slow = rb(J.slow);
    if (blockIdx.x == 0 && threadIdx.x == 0) slow[(pass + 1) & 1] = 0;
    const int sub = threadIdx.x & 15;
    const int i = blockIdx.x * FT_LEAN_PPB + (threadIdx.x >> 4);
    if (i >= J.L.N) return;
    const FtDevFrame &F = J.F;
    const bool twoCam = F.Nleft != -1;
    const unsigned long long *slotL = C.cache + (size_t)i * FT_CACHE_WORDS, *slotR = slotL + (FT_CACHE_CAP + 1);
    const uint8_t validV = rb(J.L.valid)[i];
    const unsigned long long metaL = slotL[0], metaR = twoCam ? slotR[0] : KEY_NONE;
    // (as in k_search_local_lean: the first 16 keys of both lists with the meta words, their lock records in one further trip)
    const unsigned long long keyL0 = slotL[1 + sub], keyR0 = twoCam ? slotR[1 + sub] : KEY_NONE;
    const int headL0 = metaL == KEY_NONE ? 0 : min(cache_head(metaL), FT_CACHE_CAP), headR0 = metaR == KEY_NONE ? 0 : min(cache_head(metaR), FT_CACHE_CAP);
    const bool haveL0 = sub < headL0, haveR0 = sub < headR0;
    const int kpL0 = haveL0 ? key_idx(keyL0) : 0, kpR0 = haveR0 ? key_idx(keyR0) + F.Nleft : 0;
    const LockRec recL0 = lock_record(C, kpL0), recR0 = lock_record(C, kpR0);
    int primL = -1, primR = -1;
    if (validV) {
        int nCachedL = 0, nCachedR = 0;
        bool anyBoxL = false, anyBoxR = false;
        bool fromCache = false;
        if (cache_state_of(metaL, nCachedL, anyBoxL) == 1) fromCache = !twoCam || !anyBoxL || cache_state_of(metaR, nCachedR, anyBoxR) == 1;
        if (!fromCache) {
            if (sub == 0) slow_append(slow, pass, J.nPoints, i);
            return;
        }
        auto scanMin = [&](const unsigned long long *slot, int from, int to, int base) -> unsigned long long {
            unsigned long long m = KEY_NONE;
            for (int t = from + sub; t < to; t += 16) {
                const unsigned long long key = slot[1 + t];
                if (is_locked(C, key_idx(key) + base, i, key_held(key))) continue;
                m = key < m ? key : m;
            }
            return row_min_u64(m);
        };
        // the head of the list first (cache_partition): an unlocked key there is smaller than every key behind it
        const int headL = cache_head(metaL);
        const unsigned long long firstL = (haveL0 && !locked_by(C, recL0, kpL0, i, key_held(keyL0))) ? keyL0 : KEY_NONE;
        unsigned long long k0 = headL > 16 ? scanMin(slotL, 16, headL, 0) : KEY_NONE;
        {
            const unsigned long long m = row_min_u64(firstL);
            k0 = m < k0 ? m : k0;
        }
        if (k0 == KEY_NONE && headL < nCachedL) k0 = scanMin(slotL, headL, nCachedL, 0);
        if (anyBoxL) {
            if (k0 != KEY_NONE && key_dist(k0) <= FT_TH_HIGH) primL = key_idx(k0);
            if (twoCam) {
                const int headR = cache_head(metaR);
                const unsigned long long firstR = (haveR0 && !locked_by(C, recR0, kpR0, i, key_held(keyR0))) ? keyR0 : KEY_NONE;
                unsigned long long kr = headR > 16 ? scanMin(slotR, 16, headR, F.Nleft) : KEY_NONE;
                {
                    const unsigned long long m = row_min_u64(firstR);
                    kr = m < kr ? m : kr;
                }
                if (kr == KEY_NONE && headR < nCachedR) kr = scanMin(slotR, headR, nCachedR, F.Nleft);
                if (kr != KEY_NONE && key_dist(kr) <= FT_TH_HIGH) primR = key_idx(kr) + F.Nleft;
            }
        }
    }
    const int r4[4] = {primL, -1, primR, -1};
    claims_file_row(C, res, i, sub, r4);
}

// ---- the candidate lists of a first pass, best candidates first -------------------------------------------------------------
// (the head's length goes into the meta word, see FT_CACHE_HEAD in search_dev.h)
// (PER = keys per lane: 64 PER >= n)
template <int PER>
__device__ __forceinline__ int cache_partition(unsigned long long *slot, int n, int lane) {
    unsigned long long k[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) k[j] = (lane + 64 * j < n) ? slot[1 + lane + 64 * j] : KEY_NONE;
    int lo = 0, hi = 256;  // smallest D in [0, 256] with count(dist <= D) >= FT_CACHE_HEAD (every distance is <= 256)
    while (lo < hi) {      // wave-uniform
        const int mid = (lo + hi) >> 1;
        int c = 0;
#pragma unroll
        for (int j = 0; j < PER; j++) c += (k[j] != KEY_NONE && key_dist(k[j]) <= mid) ? 1 : 0;
        if (wave_sum_i32(c) >= FT_CACHE_HEAD) hi = mid;
        else lo = mid + 1;
    }
    int c = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) c += (k[j] != KEY_NONE && key_dist(k[j]) <= lo) ? 1 : 0;
    const int head = wave_sum_i32(c);
    if (head > FT_CACHE_HEAD_MAX || head >= n) return n;
    int front = 0, back = head;  // next free position of the two parts
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const bool have = k[j] != KEY_NONE, sel = have && key_dist(k[j]) <= lo;
        const unsigned long long bs = __ballot(sel), bo = __ballot(have && !sel);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (sel) slot[1 + front + __popcll(bs & below)] = k[j];
        else if (have) slot[1 + back + __popcll(bo & below)] = k[j];
        front += __popcll(bs);
        back += __popcll(bo);
    }
    return head;
}

// the candidate lists the first pass of a batch filed: the best candidates to the front (cache_partition).  A wave takes
// FT_PART_LISTS lists one after the other (their meta words requested together: most lists are short and need nothing - a wave
// per list was bound by the rate waves can be launched at), with as many keys per lane as the list's length asks for
#define FT_PART_LISTS 4
__global__ __launch_bounds__(256) void k_cache_partition_batch(const FtBatchJob *__restrict__ jobs, Rebase rb) {
    const FtBatchJob &J = jobs[blockIdx.y];
    const int lane = threadIdx.x & 63, li0 = (blockIdx.x * 4 + wave_index()) * FT_PART_LISTS;
    const int nLists = 2 * J.nPoints;
    if (li0 >= nLists) return;
    unsigned long long *cache = rb(J.cache);
    auto slot_of = [&](int li) { return cache + (size_t)(li >> 1) * FT_CACHE_WORDS + (size_t)(li & 1) * (FT_CACHE_CAP + 1); };
    unsigned long long metas[FT_PART_LISTS];
#pragma unroll
    for (int k = 0; k < FT_PART_LISTS; k++) metas[k] = li0 + k < nLists ? slot_of(li0 + k)[0] : KEY_NONE;
#pragma unroll
    for (int k = 0; k < FT_PART_LISTS; k++) {
        const unsigned long long meta = metas[k];
        int n;
        bool anyBox;
        if (cache_state_of(meta, n, anyBox) != 1 || n <= FT_CACHE_HEAD_MAX || cache_head(meta) != n) continue;  // (wave-uniform)
        unsigned long long *slot = slot_of(li0 + k);
        int head;
        if (n <= 128) head = cache_partition<2>(slot, n, lane);
        else if (n <= 256) head = cache_partition<4>(slot, n, lane);
        else head = cache_partition<(FT_CACHE_CAP + 63) / 64>(slot, n, lane);
        if (lane == 0) slot[0] = (meta & ~(0x3ffull << 40)) | ((unsigned long long)(unsigned)head << 40);
    }
}

}  // namespace

// the first pass with four points per wave (k_search_*_first): needs the candidate cache and the grid of every frame
int ft_launch_search_last_first(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints, float th) {
    if (nFrames <= 0 || maxPoints <= 0) return FT_OK;
    const int rc = ft_launch_last_project_batch(st, arena, jobs, nFrames, maxPoints);  // (kernels_search.hip)
    if (rc != FT_OK) return rc;
    dim3 grid;
    const FtSlotGrid sg = ft_slot_grid((maxPoints + 15) / 16, nFrames, grid);  // (a frame's workgroups on one XCD: its grid and its lists stay in that L2)
    hipLaunchKernelGGL(k_search_last_first, grid, dim3(256), 0, st, jobs, rebase_of(arena), th, sg);
    FT_HIP(hipGetLastError());
    return FT_OK;
}
int ft_launch_search_local_first(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints, float th, float nnRatio) {
    if (nFrames <= 0 || maxPoints <= 0) return FT_OK;
    dim3 grid;
    const FtSlotGrid sg = ft_slot_grid((maxPoints + 15) / 16, nFrames, grid);
    hipLaunchKernelGGL(k_search_local_first, grid, dim3(256), 0, st, jobs, rebase_of(arena), th, nnRatio, sg);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

// a later pass: the lean kernel for the points the candidate cache serves, the general kernel for its slow list
int ft_launch_search_last_batch_lean(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints, int pass, int fCur,
                                     int fPrev, int fReset, float th) {
    if (nFrames <= 0 || maxPoints <= 0) return FT_OK;
    hipLaunchKernelGGL(k_search_last_lean, dim3((maxPoints + FT_LEAN_PPB - 1) / FT_LEAN_PPB, nFrames), dim3(256), 0, st, jobs,
                       rebase_of(arena), pass, fCur, fPrev, fReset);
    return ft_launch_search_last_batch_slow(st, arena, jobs, nFrames, pass, fCur, fPrev, fReset, th);  // (kernels_search.hip; checks both launches)
}

int ft_launch_search_local_batch_lean(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints, int pass, int fCur,
                                      int fPrev, int fReset, float th, float nnRatio) {
    if (nFrames <= 0 || maxPoints <= 0) return FT_OK;
    hipLaunchKernelGGL(k_search_local_lean, dim3((maxPoints + FT_LEAN_PPB - 1) / FT_LEAN_PPB, nFrames), dim3(256), 0, st, jobs,
                       rebase_of(arena), pass, fCur, fPrev, fReset, nnRatio);
    return ft_launch_search_local_batch_slow(st, arena, jobs, nFrames, pass, fCur, fPrev, fReset, th, nnRatio);
}

int ft_launch_cache_partition_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints) {
    if (nFrames <= 0 || maxPoints <= 0) return FT_OK;
    hipLaunchKernelGGL(k_cache_partition_batch, dim3((2 * maxPoints + 4 * FT_PART_LISTS - 1) / (4 * FT_PART_LISTS), nFrames), dim3(256), 0, st, jobs,
                       rebase_of(arena));
    FT_HIP(hipGetLastError());
    return FT_OK;
}

// HIP kernels that finish the projection searches of a batch of frames (ft_tracked_batch) on the device, a workgroup per frame
// (gfx950, wave64) - EXPERIMENTS.md sections 10.7 and 11.9:
//   k_resolve_batch  the claim iteration behind the first pass in ONE launch: the points of a frame in index order, a chunk at a
//                    time - the in-call claiming of ORBmatcher::SearchByProjection (reference src/ORBmatcher.cc:101-103, 142)
//   k_replay_batch   the writes of a converged search: mvpMapPoints in point order, the rotation histogram, ComputeThreeMaxima
//                    (src/ORBmatcher.cc:134-148, 1860-1896, 1966-1987, 2210-2251)
// Both read the candidate lists and results the search kernels left (kernels_search_rows.hip, kernels_search.hip); the key and
// the meta word of a list are search_dev.h's.
#include <climits>

#include "search_dev.h"

namespace {

// ---- a batch's claims resolved in ONE launch: the points of a frame in index order, a chunk at a time --------------------------
// The claim passes (kernels_search.hip, kernels_search_rows.hip) are a Jacobi iteration over ALL points of a frame: a point's locks depend on the writes of the points in
// front of it, a dependency chain of length c takes c passes, and every pass re-evaluates every point (13 - 20 passes of a batch
// at configs[3]).  But the dependency is triangular, and a batch has parallelism to spare ACROSS its frames.  So: one workgroup
// per frame walks the frame's points in index order, FT_RS_ROWS at a time (a point = a row of 16 lanes, as in the lean kernels).
// When a chunk is evaluated every point in front of it is FINAL: of their writes a keypoint needs to remember only the last
// (lastW[kp], an atomicMax of the writer-table entry: the largest (4 point + kind) - what locked_by picks from a record), and
// only the writes of the chunk's own points are still in motion - they are iterated inside the workgroup, on a hash table in
// LDS (keypoint -> bit mask of the chunk's rows that write it), until an iteration changes nothing.  An iteration after the
// first touches LDS only (keys and lastW values stay in registers).  A point is evaluated 2 - 3 times instead of 13 - 20, and
// a search is the first pass (window scans, k_search_*_first), the partition of the lists and this.
// It reads the candidate lists the first pass filed; a point whose list is not usable (more candidates than the cache holds)
// makes the workgroup give up on its frame: the frame's flag words stay as the first pass left them, the host sees it and
// continues with the claim passes for such frames (resolved frames are inert there: all their flag words read "converged").
#ifndef FT_RS_W
#define FT_RS_W 16                       // lanes per point (a GROUP of lanes inside a DPP row): 16 or 8
#endif
#define FT_RS_LANES 1024                 // a workgroup
#define FT_RS_ROWS (FT_RS_LANES / FT_RS_W)   // points per chunk: 64 (128 with 8 lanes per point)
#define FT_RS_SLOTS (8 * FT_RS_ROWS)     // hash slots (<= 4 writes per point and chunk): a power of two
#define FT_RS_REG (48 / FT_RS_W)         // keys of a list's head a lane keeps in registers (x FT_RS_W lanes = FT_CACHE_HEAD_MAX)
#define FT_RS_MW (FT_RS_ROWS / 32)       // 32-bit words of a row mask
static_assert((FT_RS_W == 8 || FT_RS_W == 16) && FT_RS_W * FT_RS_REG == FT_CACHE_HEAD_MAX, "k_resolve_batch: a point is 8 or 16 lanes");
// (Round 6 measured 8 lanes per point - eight points per wave, 16 chunks of 128 points instead of 32 of 64: the last-frame
// resolution took the same 0.24 ms, the local-map one 0.63 instead of 0.46 (th 15: 0.50 / 1.20 against 0.41 / 0.94) - twice the
// points per chunk are more than twice the chunk: more of them collide inside it (more iterations), and six key registers per
// lane and camera spill.  EXPERIMENTS 11.9.)
struct RsShared {
    // two hash tables used alternately by the iterations of a chunk (iteration `it` reads table it & 1 and clears the other
    // one for its successor): keypoint -> rows of the chunk that write it (their results of the previous iteration)
    int kp[2][FT_RS_SLOTS];
    unsigned mask[2][FT_RS_MW][FT_RS_SLOTS];
    unsigned char obs[FT_RS_ROWS];  // Observations() > 0 of the chunk's points
    int vote[3];                    // "iteration it changed a result", slot it % 3
};
__device__ __forceinline__ unsigned rs_hash(int kp) { return ((unsigned)kp * 2654435761u) >> (32 - __builtin_ctz(FT_RS_SLOTS)); }
__device__ __forceinline__ void rs_clear(RsShared &S, int t) {
    for (int k = threadIdx.x; k < FT_RS_SLOTS; k += FT_RS_LANES) {
        S.kp[t][k] = -1;
#pragma unroll
        for (int w = 0; w < FT_RS_MW; w++) S.mask[t][w][k] = 0u;
    }
}
// a barrier for what the workgroup exchanges through LDS: outstanding loads from memory (the next chunk's prefetch) stay outstanding
__device__ __forceinline__ void rs_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
__device__ __forceinline__ void rs_insert(RsShared &S, int t, int kp, int row) {
    unsigned h = rs_hash(kp);
    for (;;) {
        const int old = atomicCAS(&S.kp[t][h], -1, kp);
        if (old == -1 || old == kp) break;
        h = (h + 1) & (FT_RS_SLOTS - 1);
    }
    atomicOr(&S.mask[t][row >> 5][h], 1u << (row & 31));
}
// F.mvpMapPoints[kp] && ->Observations() > 0 as the point of row `row` sees it: the last writer in front of it - of this chunk
// (hash table t; useHash = 0: the chunk's first iteration, no writes of the chunk yet) or, if none, of the chunks before (lw = lastW[kp]) -
// decides, else the pre-call holder
__device__ __forceinline__ bool rs_locked(const RsShared &S, int t, bool useHash, int kp, int lw, bool held, int row) {
    if (useHash) {
        unsigned h = rs_hash(kp);
        for (;;) {
            const int k = S.kp[t][h];
            if (k == -1) break;
            if (k == kp) {
                // the highest row below `row` that writes the keypoint: the word of `row` cut off at its bit, then the words below
                int w = row >> 5;
                unsigned m = S.mask[t][w][h] & ((1u << (row & 31)) - 1u);
                while (m == 0u && w > 0) m = S.mask[t][--w][h];
                if (m) return S.obs[32 * w + 31 - __clz((int)m)] != 0;
                break;
            }
            h = (h + 1) & (FT_RS_SLOTS - 1);
        }
    }
    return lw >= 0 ? (lw & 1) != 0 : held;
}
// minima / maxima over the FT_RS_W lanes of a point, in every lane of it: DPP steps that stay inside the group (lane pairs, quads,
// halves of a row - and, for sixteen lanes, the row)
__device__ __forceinline__ unsigned long long grp_min_u64(unsigned long long v) {
#define FT_MIN64_STEP(ctrl)                                                                                   \
    {                                                                                                         \
        const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, ctrl, 0xF, 0xF, true); \
        const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(v >> 32), ctrl, 0xF, 0xF, true);   \
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;                                     \
        v = w < v ? w : v;                                                                                    \
    }
    FT_MIN64_STEP(0xB1) FT_MIN64_STEP(0x4E) FT_MIN64_STEP(0x141)
    if constexpr (FT_RS_W == 16) FT_MIN64_STEP(0x140)
#undef FT_MIN64_STEP
    return v;
}
__device__ __forceinline__ int grp_max_i32(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));
    if constexpr (FT_RS_W == 16) v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));
    return v;
}
__device__ __forceinline__ void grp_two_min(unsigned long long &k0, unsigned long long &k1) {
    const unsigned long long m0 = grp_min_u64(k0);
    const unsigned long long cand = (k0 == m0) ? k1 : k0;
    k1 = grp_min_u64(cand);
    k0 = m0;
}
// The last writers of the points in front of the running chunk, one word per keypoint of the frame.  LWLDS (round 6): the table
// lives in the workgroup's LDS for the whole walk (F.N ints: 16 KB at configs[3]) - a chunk's publication is an LDS atomic and
// the next chunk's look-ups are LDS reads, where round 5 went through L2 both ways (atomicMax, then device-scope loads that had
// to wait for it: one memory round trip on every chunk's critical path, 32 chunks per frame).  Frames too large for the LDS
// keep the table in HBM (buffer 0 of the list heads).
template <bool LWLDS>
__device__ __forceinline__ int rs_last_writer(const int *lastW, int kp) {
    if constexpr (LWLDS) return lastW[kp];
    else return __hip_atomic_load(lastW + kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// results of a converged chunk: both result buffers (the host reads the one of the parity it is told), lastW for the chunks behind
__device__ __forceinline__ void rs_publish(int *res0, int *res1, int *lastW, int i, int sub, bool obsI, const int r4[4]) {
    if (sub < 4) {
        const int kp = sub == 0 ? r4[0] : sub == 1 ? r4[1] : sub == 2 ? r4[2] : r4[3];
        const int s = 4 * i + sub;
        res0[s] = kp;
        res1[s] = kp;
        if (kp >= 0) atomicMax(lastW + kp, (s << 1) | (obsI ? 1 : 0));  // (LDS or HBM: the address space decides the instruction)
    }
}
// what a point's turn needs that no other point's result changes - requested a chunk ahead
struct RsStatic {
    unsigned long long metaL, metaR, kL[FT_RS_REG], kR[FT_RS_REG];
    int obs;
    unsigned char f0, f1, f2;  // local map: skip, inView, inViewR; last frame: valid
    int levelR;
};
template <bool LOCAL>
__device__ __forceinline__ RsStatic rs_fetch(const FtBatchJob &J, const Rebase &rb, const unsigned long long *cache, const int *obsP, bool twoCam,
                                             int i, int sub) {
    RsStatic T;
    const unsigned long long *slotL = cache + (size_t)i * FT_CACHE_WORDS, *slotR = slotL + (FT_CACHE_CAP + 1);
    T.metaL = slotL[0];
    T.metaR = twoCam ? slotR[0] : KEY_NONE;
#pragma unroll
    for (int j = 0; j < FT_RS_REG; j++) {  // (whatever the lists' lengths: a key beyond a head is dropped when the meta word is there)
        T.kL[j] = slotL[1 + sub + FT_RS_W * j];
        T.kR[j] = twoCam ? slotR[1 + sub + FT_RS_W * j] : KEY_NONE;
    }
    T.obs = obsP[i];
    T.levelR = -1;
    if constexpr (LOCAL) {
        T.f0 = rb(J.P.skip)[i];
        T.f1 = rb(J.P.inView)[i];
        T.f2 = twoCam ? rb(J.P.inViewR)[i] : (unsigned char)0;
        if (twoCam) T.levelR = rb(J.P.levelR)[i];
    } else {
        T.f0 = rb(J.L.valid)[i];
        T.f1 = T.f2 = 0;
    }
    return T;
}

template <bool LOCAL, bool LWLDS>
__global__ __launch_bounds__(FT_RS_LANES) void k_resolve_batch(const FtBatchJob *__restrict__ jobs, Rebase rb, float nnRatio) {
    const FtBatchJob &J = jobs[blockIdx.x];
    if (J.nPoints <= 0) return;
    __shared__ RsShared S;
    extern __shared__ int rs_lw[];  // LWLDS: the frame's last-writer table
    const FtDevFrame &F = J.F;
    const bool twoCam = F.Nleft != -1;
    const int M = LOCAL ? J.P.M : J.L.N;
    const int row = threadIdx.x / FT_RS_W, sub = threadIdx.x % FT_RS_W;
    int *res0 = rb(J.res), *res1 = res0 + 4 * (size_t)J.nPoints;
    // (HBM form: buffer 0 of the list heads, all -1 after k_fill_claims_batch and not written by a first pass)
    int *lastW = LWLDS ? rs_lw : rb(J.head);
    if constexpr (LWLDS)
        for (int k = threadIdx.x; k < F.N; k += FT_RS_LANES) rs_lw[k] = -1;  // (the pre-scan's barrier below orders it)
    const int *obsP = rb(J.obs);
    const unsigned long long *cache = rb(J.cache);
    const int *l2r = rb(F.l2r), *r2l = rb(F.r2l);
    if (threadIdx.x < 3) S.vote[threadIdx.x] = 0;
    rs_clear(S, 1);  // (the table of a chunk's second iteration; the pre-scan's barrier below orders it)
    RsStatic T = rs_fetch<LOCAL>(J, rb, cache, obsP, twoCam, min(row, M - 1), sub);
    // Usable or not is decided for the WHOLE frame before the first chunk publishes anything (results, last writers): the meta
    // words of every list the frame's points will want, a point per lane.  A frame the kernel gives up on is untouched - the
    // claim passes that take over read the first pass's results and an all -1 last-writer buffer, as if this kernel had not run.
    // (Round 5 tested chunk by chunk: a list beyond the cache in a later chunk left the earlier chunks published.)
    {
        bool unusable = false;
        for (int p = threadIdx.x; p < M; p += FT_RS_LANES) {
            const unsigned long long *slotL = cache + (size_t)p * FT_CACHE_WORDS;
            const unsigned long long mL = slotL[0], mR = twoCam ? slotL[FT_CACHE_CAP + 1] : KEY_NONE;
            int nL = 0, nR = 0;
            bool boxL = false, boxR = false;
            const int stL = cache_state_of(mL, nL, boxL), stR = cache_state_of(mR, nR, boxR);
            bool wantL, wantR;
            if constexpr (LOCAL) {
                const bool skip = rb(J.P.skip)[p] != 0;
                wantL = !skip && rb(J.P.inView)[p] != 0;
                wantR = !skip && twoCam && rb(J.P.inViewR)[p] != 0 && rb(J.P.levelR)[p] != -1;
            } else {
                wantL = rb(J.L.valid)[p] != 0;
                wantR = wantL && twoCam && stL == 1 && boxL;
            }
            unusable = unusable || (wantL && stL != 1) || (wantR && stR != 1);
        }
        if (__syncthreads_or(unusable ? 1 : 0)) return;  // (the frame's flag words untouched: the host goes on with the passes)
    }
    for (int base = 0; base < M; base += FT_RS_ROWS) {  // (uniform)
        const int i = base + row;
        const bool act = i < M;
        const int ii = act ? i : M - 1;
        const unsigned long long *slotL = cache + (size_t)ii * FT_CACHE_WORDS, *slotR = slotL + (FT_CACHE_CAP + 1);
        bool wantL, wantR;
        if constexpr (LOCAL) {
            wantL = act && !T.f0 && T.f1;
            wantR = act && !T.f0 && twoCam && T.f2 && T.levelR != -1;
        } else {
            wantL = act && T.f0;
            wantR = wantL && twoCam;
        }
        const bool obsI = T.obs > 0;
        int nL = 0, nR = 0;
        bool anyBoxL = false, anyBoxR = false;
        const int stL = cache_state_of(T.metaL, nL, anyBoxL), stR = cache_state_of(T.metaR, nR, anyBoxR);
        (void)stR;
        if constexpr (!LOCAL) wantR = wantR && stL == 1 && anyBoxL;  // (`if(vIndices2.empty()) continue;` skips the right-camera block)
        const int headL = wantL ? cache_head(T.metaL) : 0, headR = wantR ? cache_head(T.metaR) : 0;
        if (!wantL) nL = 0;
        if (!wantR) nR = 0;
        unsigned long long kL[FT_RS_REG], kR[FT_RS_REG];
        int wL[FT_RS_REG], wR[FT_RS_REG], mL[FT_RS_REG], mR[FT_RS_REG];  // last writers; the keypoints' entries of the match tables
#pragma unroll
        for (int j = 0; j < FT_RS_REG; j++) {
            kL[j] = (sub + FT_RS_W * j < headL) ? T.kL[j] : KEY_NONE;
            kR[j] = (sub + FT_RS_W * j < headR) ? T.kR[j] : KEY_NONE;
        }
#pragma unroll
        for (int j = 0; j < FT_RS_REG; j++) {
            wL[j] = kL[j] != KEY_NONE ? rs_last_writer<LWLDS>(lastW, key_idx(kL[j])) : -1;
            wR[j] = kR[j] != KEY_NONE ? rs_last_writer<LWLDS>(lastW, key_idx(kR[j]) + F.Nleft) : -1;
            mL[j] = mR[j] = -1;
            if constexpr (LOCAL) {
                if (twoCam) {
                    if (kL[j] != KEY_NONE) mL[j] = l2r[key_idx(kL[j])];
                    if (kR[j] != KEY_NONE) mR[j] = r2l[key_idx(kR[j])];
                }
            }
        }
        if (base + FT_RS_ROWS < M) T = rs_fetch<LOCAL>(J, rb, cache, obsP, twoCam, min(i + FT_RS_ROWS, M - 1), sub);  // the next chunk's
        if (sub == 0) S.obs[row] = obsI ? 1 : 0;  // (read behind the barrier of the second iteration)
        if (threadIdx.x == 0) S.vote[1] = 0;      // (the second iteration's slot; the later ones are reset an iteration ahead)
        int r4[4] = {-1, -1, -1, -1};
        int it = 0;
        for (;; it++) {  // (uniform)
            const bool useHash = it > 0;
            const int ht = it & 1;
            // Two barriers per iteration behind the first: table ht is CLEAN here (cleared while the iteration before the last
            // one - or the previous chunk - was inserting: a barrier ago at least), the rows file their writes of the previous
            // iteration in it and clear the other table for the next iteration, barrier, everybody evaluates against it, barrier,
            // the vote.  (Round 5: one table, cleared between two barriers of its own - four barriers per iteration.)
            if (it > 0) {
                if (act && sub < 4) {
                    const int kp = sub == 0 ? r4[0] : sub == 1 ? r4[1] : sub == 2 ? r4[2] : r4[3];
                    if (kp >= 0) rs_insert(S, ht, kp, row);
                }
                rs_clear(S, ht ^ 1);
                if (threadIdx.x == 0) S.vote[(it + 1) % 3] = 0;  // (slot of the next iteration: last read two barriers ago)
                rs_barrier();
            }
            int primL = -1, sideL = -1, primR = -1, sideR = -1;
            if constexpr (LOCAL) {
                bool skipRight = false;
                if (wantL) {
                    unsigned long long k0 = KEY_NONE, k1 = KEY_NONE;
#pragma unroll
                    for (int j = 0; j < FT_RS_REG; j++)
                        if (kL[j] != KEY_NONE && !rs_locked(S, ht, useHash, key_idx(kL[j]), wL[j], key_held(kL[j]), row)) two_min_insert(k0, k1, kL[j]);
                    auto scan = [&](int from, int to) {
                        for (int t = from + sub; t < to; t += FT_RS_W) {
                            const unsigned long long key = slotL[1 + t];
                            const int kp = key_idx(key);
                            if (rs_locked(S, ht, useHash, kp, rs_last_writer<LWLDS>(lastW, kp), key_held(key), row)) continue;
                            two_min_insert(k0, k1, key);
                        }
                    };
                    if (headL > FT_RS_W * FT_RS_REG) scan(FT_RS_W * FT_RS_REG, headL);
                    grp_two_min(k0, k1);
                    if (k1 == KEY_NONE && headL < nL) {  // fewer than two unlocked keys in the head: the rest of the list decides
                        scan(headL, nL);
                        grp_two_min(k0, k1);
                    }
                    int bd = 256, bd2 = 256, bl = -1, bl2 = -1, bi = -1;
                    if (k0 != KEY_NONE) { bd = key_dist(k0); bi = key_idx(k0); bl = key_octave(k0); }
                    if (k1 != KEY_NONE) { bd2 = key_dist(k1); bl2 = key_octave(k1); }
                    if (bd <= FT_TH_HIGH) {
                        if (bl == bl2 && (float)bd > __fmul_rn(nnRatio, (float)bd2)) skipRight = true;
                        else {
                            primL = bi;
                            if (twoCam) {  // l2r[bi]: with the winner's lane, or (a key from beyond the registers) in memory
                                int m = INT_MIN;
#pragma unroll
                                for (int j = 0; j < FT_RS_REG; j++) m = kL[j] == k0 ? mL[j] : m;
                                m = grp_max_i32(m);
                                if (m == INT_MIN) m = l2r[bi];
                                if (m != -1) sideL = m + F.Nleft;
                            }
                        }
                    }
                }
                if (wantR && !skipRight) {
                    unsigned long long k0 = KEY_NONE, k1 = KEY_NONE;
                    // this point's own left-block side write precedes its right-block search
                    auto lockedR = [&](int g, int lw, bool held) -> bool { return (g == sideL) ? obsI : rs_locked(S, ht, useHash, g, lw, held, row); };
#pragma unroll
                    for (int j = 0; j < FT_RS_REG; j++)
                        if (kR[j] != KEY_NONE && !lockedR(key_idx(kR[j]) + F.Nleft, wR[j], key_held(kR[j]))) two_min_insert(k0, k1, kR[j]);
                    auto scan = [&](int from, int to) {
                        for (int t = from + sub; t < to; t += FT_RS_W) {
                            const unsigned long long key = slotR[1 + t];
                            const int g = key_idx(key) + F.Nleft;
                            if (lockedR(g, rs_last_writer<LWLDS>(lastW, g), key_held(key))) continue;
                            two_min_insert(k0, k1, key);
                        }
                    };
                    if (headR > FT_RS_W * FT_RS_REG) scan(FT_RS_W * FT_RS_REG, headR);
                    grp_two_min(k0, k1);
                    if (k1 == KEY_NONE && headR < nR) {
                        scan(headR, nR);
                        grp_two_min(k0, k1);
                    }
                    int bdr = 256, bd2r = 256, blr = -1, bl2r = -1, bir = -1;
                    if (k0 != KEY_NONE) { bdr = key_dist(k0); bir = key_idx(k0); blr = key_octave(k0); }
                    if (k1 != KEY_NONE) { bd2r = key_dist(k1); bl2r = key_octave(k1); }
                    if (bdr <= FT_TH_HIGH && !(blr == bl2r && (float)bdr > __fmul_rn(nnRatio, (float)bd2r))) {
                        int m = INT_MIN;
#pragma unroll
                        for (int j = 0; j < FT_RS_REG; j++) m = kR[j] == k0 ? mR[j] : m;
                        m = grp_max_i32(m);
                        if (m == INT_MIN) m = r2l[bir];
                        if (m != -1) sideR = m;
                        primR = bir + F.Nleft;
                    }
                }
            } else {
                auto listMin = [&](const unsigned long long *slot, const unsigned long long *kReg, const int *wReg, int head, int n, int off) {
                    unsigned long long m = KEY_NONE;
#pragma unroll
                    for (int j = 0; j < FT_RS_REG; j++)
                        if (kReg[j] != KEY_NONE && !rs_locked(S, ht, useHash, key_idx(kReg[j]) + off, wReg[j], key_held(kReg[j]), row))
                            m = kReg[j] < m ? kReg[j] : m;
                    auto scan = [&](int from, int to) {
                        for (int t = from + sub; t < to; t += FT_RS_W) {
                            const unsigned long long key = slot[1 + t];
                            const int g = key_idx(key) + off;
                            if (rs_locked(S, ht, useHash, g, rs_last_writer<LWLDS>(lastW, g), key_held(key), row)) continue;
                            m = key < m ? key : m;
                        }
                    };
                    if (head > FT_RS_W * FT_RS_REG) scan(FT_RS_W * FT_RS_REG, head);
                    m = grp_min_u64(m);
                    // the head of the list first (cache_partition): an unlocked key there is smaller than every key behind it
                    if (m == KEY_NONE && head < n) {
                        scan(head, n);
                        m = grp_min_u64(m);
                    }
                    return m;
                };
                if (wantL && anyBoxL) {
                    const unsigned long long k0 = listMin(slotL, kL, wL, headL, nL, 0);
                    if (k0 != KEY_NONE && key_dist(k0) <= FT_TH_HIGH) primL = key_idx(k0);
                    if (wantR) {
                        const unsigned long long kr = listMin(slotR, kR, wR, headR, nR, F.Nleft);
                        if (kr != KEY_NONE && key_dist(kr) <= FT_TH_HIGH) primR = key_idx(kr) + F.Nleft;
                    }
                }
            }
            const bool changed = act && (primL != r4[0] || sideL != r4[1] || primR != r4[2] || sideR != r4[3]);
            r4[0] = primL; r4[1] = sideL; r4[2] = primR; r4[3] = sideR;
            if (it == 0) continue;  // (the first iteration's results are what the second one starts from, changed or not)
            if (changed && sub == 0) S.vote[it % 3] = 1;
            rs_barrier();
            if (!S.vote[it % 3]) break;
#ifdef FT_RS_MAXIT
            if (it >= FT_RS_MAXIT) break;
#endif
        }
#ifndef FT_RS_NOPUB
        if (act) rs_publish(res0, res1, lastW, i, sub, obsI, r4);
#endif
        // The next chunk's rs_last_writer loads must see this chunk's atomicMax.  Both are device-scope operations that execute in
        // L2 (the atomic there, the sc1 load from there), issued by waves of ONE workgroup = one CU, and what orders them is the
        // CU's in-order vector-memory path: the ISA of the fence + barrier below is `s_waitcnt lgkmcnt(0) ; s_barrier` - NO
        // `vmcnt(0)`, the workgroup-scope release waits for nothing of the atomics - so a load issued behind the barrier is behind
        // every atomic issued in front of it in the same CU's queue to the same L2 channel (the same address).  LLVM's AMDGPU
        // memory model guarantees that order only in non-threadgroup-split mode (tgsplit: the waves of a workgroup may sit on
        // different CUs and a workgroup-scope release becomes a real wait); the build refuses tgsplit (csrc/Makefile: check-tgsplit,
        // tests/test_build_flags.py - the compiler defines no macro a static_assert could test).  An
        // agent-scope fence (__threadfence) would be safe everywhere and writes the L2 back, 30 us a time (EXPERIMENTS 10.7).
        // The next chunk's second iteration files into table 1: dirty when this chunk ended in an odd iteration (an even one cleared it)
        if (it & 1) rs_clear(S, 1);
        // (LWLDS: the table is in LDS - an LDS-only barrier, and none of the above applies)
        if constexpr (LWLDS) rs_barrier();
        else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __syncthreads();
        }
    }
    // resolved: every flag word of the frame reads "converged"
    int *flags = rb(J.flags);
    if (threadIdx.x < FT_BATCH_FLAGS) flags[threadIdx.x] = -1;
}

// ---- the writes of a converged search, replayed where the results are ------------------------------------------------------------
// What the host did with a search's results until round 5 (replayLocalWrites / replayLastFrameWrites, search_host.h) - and what
// the reference does while it searches: CurrentFrame.mvpMapPoints[kp] = pMP in point order (src/ORBmatcher.cc:134-148, 203-214;
// 1860-1879, 1934-1941), the rotation histogram (:1880-1896, 1942-1957), ComputeThreeMaxima (:2210-2251) and the removal of
// the matches outside the three dominant bins (:1966-1987).  A workgroup per frame:
//   assign[kp]  = the LAST point that wrote keypoint kp (atomicMax of the point index over all writes), -1 if none - or if ANY
//                 write to kp fell into a removed histogram bin (the reference clears mvpMapPoints[kp] for every entry of such a bin,
//                 whoever wrote the keypoint last);
//   holder[kp]  = Observations() of that point, -1 where the histogram removed the keypoint, unchanged where nobody wrote;
//   nm          = writes - writes in removed bins (nmatches++ per write, nmatches-- per removed entry).
// The frame's holder_obs stays in HBM (the next search of the batch reads it there), assign and nm go straight into pinned host
// memory.  The last-writer table lives in LDS (F.N ints) or, for frames beyond it, in the frame's writer table (dead by now).
#define FT_REPLAY_REMOVED 0x40000000
template <bool LOCAL, bool INLDS>
__global__ __launch_bounds__(256) void k_replay_batch(const FtBatchJob *__restrict__ jobs, Rebase rb, int parity, int checkOrientation,
                                                      int flagPos) {
    const FtBatchJob &J = jobs[blockIdx.x];
    extern __shared__ int rp_last[];
    __shared__ int rp_hist[FT_HISTO_LENGTH], rp_keep, rp_sum[4];
    int *replayed = rb(J.replayed);
    const int *flags = rb(J.flags);
    const int N = J.F.N, M = J.nPoints;
    // (uniform) a frame that has been replayed already; flagPos >= 0 (a launch enqueued before the host has seen the flag words -
    // right behind k_resolve_batch: position 0, or behind a burst of claim passes: the burst's last position): only a frame whose
    // flag word there says "converged"; the others wait for the passes still to come
    if (*replayed >= 0 || (flagPos >= 0 && M > 0 && flags[flagPos] != -1)) return;
    const int tid = threadIdx.x;
    int *last = INLDS ? rp_last : rb(J.tab);
    int *assign = J.assignOut;
    int *holder = const_cast<int *>(rb(J.F.holderObs));
    const int *res = rb(J.res) + (size_t)parity * 4 * (size_t)M;
    const int *obs = rb(J.obs);
    const bool hist = !LOCAL && checkOrientation != 0;
    const int nLk = J.F.Nleft == -1 ? N : J.F.Nleft;
    const ft_keypoint *keys = rb(J.F.keys), *keysR = rb(J.F.keysR);
    const float *lastAngle = LOCAL ? nullptr : rb(J.L.angle);
    for (int kp = tid; kp < N; kp += 256) last[kp] = -1;
    if (tid < FT_HISTO_LENGTH) rp_hist[tid] = 0;
    if (!INLDS) __threadfence();
    __syncthreads();
    // rotation bin of the write (point i -> keypoint kp): src/ORBmatcher.cc:1882-1890, the host replay's expression operation by operation
    auto bin_of = [&](int i, int kp) -> int {
        // (init_bin written out: the call costs this kernel a 17th VGPR)
        const float cur = kp < nLk ? keys[kp].angle : keysR[kp - nLk].angle;
        float rot = __fsub_rn(lastAngle[i], cur);
        if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
        int bin = (int)roundf(__fmul_rn(rot, 1.0f / FT_HISTO_LENGTH));
        if (bin == FT_HISTO_LENGTH) bin = 0;
        return bin;
    };
    int nm = 0;
    for (int s = tid; s < 4 * M; s += 256) {
        if (!LOCAL && (s & 1)) continue;  // last frame: the primary writes of the two cameras (res[4 i], res[4 i + 2])
        const int kp = res[s];
        if (kp < 0) continue;
        const int i = s >> 2;
        nm++;
        atomicMax(&last[kp], i);
        if (hist) {
            const int bin = bin_of(i, kp);
            if (bin >= 0 && bin < FT_HISTO_LENGTH) atomicAdd(&rp_hist[bin], 1);
        }
    }
    if (!INLDS) __threadfence();
    __syncthreads();
    if (hist) {
        if (tid == 0) rp_keep = three_maxima_keep(rp_hist);  // ComputeThreeMaxima (src/ORBmatcher.cc:2210-2251)
        __syncthreads();
        const int keep = rp_keep;
        for (int s = tid; s < 4 * M; s += 256) {
            if (s & 1) continue;
            const int kp = res[s];
            if (kp < 0) continue;
            const int bin = bin_of(s >> 2, kp);
            if (bin >= 0 && bin < FT_HISTO_LENGTH && !((keep >> bin) & 1)) {
                atomicMax(&last[kp], FT_REPLAY_REMOVED);
                nm--;
            }
        }
        if (!INLDS) __threadfence();
        __syncthreads();
    }
    for (int kp = tid; kp < N; kp += 256) {
        const int a = INLDS ? last[kp] : __hip_atomic_load(last + kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int out = -1;
        if (a >= FT_REPLAY_REMOVED) holder[kp] = -1;
        else if (a >= 0) {
            out = a;
            holder[kp] = obs[a];
        }
        assign[kp] = out;
    }
    nm = wave_sum_i32(nm);
    if ((tid & 63) == 0) rp_sum[tid >> 6] = nm;
    __syncthreads();
    if (tid == 0) {
        const int total = rp_sum[0] + rp_sum[1] + rp_sum[2] + rp_sum[3];
        *J.nmOut = total;
        *replayed = total;
    }
}

}  // namespace

// everything behind the first pass of a batch in one launch (k_resolve_batch): a workgroup per frame
int ft_launch_resolve_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int local, float nnRatio, int sharedInts) {
    if (nFrames <= 0) return FT_OK;
    const size_t sh = sizeof(int) * (size_t)sharedInts;  // the last-writer table of the largest frame; 0: frames beyond the LDS
    if (sharedInts > 0) {
        if (local) hipLaunchKernelGGL((k_resolve_batch<true, true>), dim3(nFrames), dim3(FT_RS_LANES), sh, st, jobs, rebase_of(arena), nnRatio);
        else hipLaunchKernelGGL((k_resolve_batch<false, true>), dim3(nFrames), dim3(FT_RS_LANES), sh, st, jobs, rebase_of(arena), nnRatio);
    } else {
        if (local) hipLaunchKernelGGL((k_resolve_batch<true, false>), dim3(nFrames), dim3(FT_RS_LANES), 0, st, jobs, rebase_of(arena), nnRatio);
        else hipLaunchKernelGGL((k_resolve_batch<false, false>), dim3(nFrames), dim3(FT_RS_LANES), 0, st, jobs, rebase_of(arena), nnRatio);
    }
    FT_HIP(hipGetLastError());
    return FT_OK;
}
int ft_launch_replay_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int local, int parity, int checkOrientation,
                           int sharedInts, int flagPos) {
    if (nFrames <= 0) return FT_OK;
    const Rebase rb = rebase_of(arena);
    const size_t sh = sizeof(int) * (size_t)sharedInts;
    if (sharedInts > 0) {
        if (local) hipLaunchKernelGGL((k_replay_batch<true, true>), dim3(nFrames), dim3(256), sh, st, jobs, rb, parity, checkOrientation, flagPos);
        else hipLaunchKernelGGL((k_replay_batch<false, true>), dim3(nFrames), dim3(256), sh, st, jobs, rb, parity, checkOrientation, flagPos);
    } else {
        if (local) hipLaunchKernelGGL((k_replay_batch<true, false>), dim3(nFrames), dim3(256), 0, st, jobs, rb, parity, checkOrientation, flagPos);
        else hipLaunchKernelGGL((k_replay_batch<false, false>), dim3(nFrames), dim3(256), 0, st, jobs, rb, parity, checkOrientation, flagPos);
    }
    FT_HIP(hipGetLastError());
    return FT_OK;
}

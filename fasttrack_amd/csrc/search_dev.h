// Device side of the projection searches: what more than one of kernels_search.hip, kernels_search_rows.hip,
// kernels_resolve.hip, kernels_frame.hip, kernels_reloc.hip, kernels_fuse.hip and kernels_sim3.hip uses - a frame's pointers, the candidate key, the claim records of a pass, the
// meta word of a candidate list, a window's entry, the camera models.  A helper that only one of those files uses lives in
// that file.  Everything here is __device__ __forceinline__ (or a type) in an anonymous namespace: nothing links across files.
// Device only: nothing includes this header except those seven .hip files.
#pragma once
#include "kb8_math.h"
#include "ft_search.h"
#include "wave_ops.h"

namespace {

// The array pointers of a frame as the scans use them.  The kernels of ONE frame get the frame as a kernel argument and
// its pointers are global pointers to the compiler; a pointer read from a record in memory (the job records of the batch
// kernels, FtBatchJob) is a GENERIC pointer - flat_load: both wait counters, an aperture check per access - and neither
// a cast through the global address space nor llvm.assume(!is_shared && !is_private) survives the optimiser.  What does:
// re-deriving the pointer from a pointer that IS a kernel argument - the batch's device arena, with the arena's address
// passed a second time as a plain integer, so that arena + (p - address) cannot be folded back into p.  Everything a job
// record points to lies inside the arena of its batch (tracked_batch.cpp).
struct NoRebase {  // the pointers are kernel arguments already
    template <class T>
    __device__ __forceinline__ T *operator()(T *p) const {
        return p;
    }
};
struct FramePtrs {
    const ft_keypoint *keys, *keysR;
    const uint8_t *desc;
    const float *uright;
    const int *holderObs, *l2r, *r2l;
    const int *gridStart[2];
    const float4 *gridRec[2];
    const uint8_t *gridDesc[2];
};
template <class RB>
__device__ __forceinline__ FramePtrs frame_ptrs(const FtDevFrame &F, const RB &rb) {
    FramePtrs Q;
    Q.keys = rb(F.keys); Q.keysR = rb(F.keysR); Q.desc = rb(F.desc); Q.uright = rb(F.uright);
    Q.holderObs = rb(F.holderObs); Q.l2r = rb(F.l2r); Q.r2l = rb(F.r2l);
    Q.gridStart[0] = rb(F.gridStart[0]); Q.gridStart[1] = rb(F.gridStart[1]);
    Q.gridRec[0] = rb(F.gridRec[0]); Q.gridRec[1] = rb(F.gridRec[1]);
    Q.gridDesc[0] = rb(F.gridDesc[0]); Q.gridDesc[1] = rb(F.gridDesc[1]);
    return Q;
}
#define FT_NO_REBASE (NoRebase{})

#define KEY_NONE 0xffffffffffffffffull
// Candidate key: (distance, cell x, cell y, index) in the high bits - ascending keys are the scan order of the CPU loop, see
// the header of kernels_search.hip - and below them what a later pass would otherwise have to fetch again through dependent loads: the keypoint's
// octave (four bits: checkFrame, search_host.h, admits octaves of [0, nlevels) only; masked here so that the keypoints of a
// BOUND frame, which no host check sees, can never spill into the index) and whether it was held before the call
// (mvpMapPoints[idx]->Observations() > 0).  The index is unique inside a window, so the low bits never decide a comparison.
__device__ __forceinline__ unsigned long long make_key(int dist, int cx, int cy, int idx, int octave, bool heldBefore) {
    return ((unsigned long long)dist << 41) | ((unsigned long long)cx << 35) | ((unsigned long long)cy << 29) |
           ((unsigned long long)idx << 5) | ((unsigned long long)(octave & 15) << 1) | (heldBefore ? 1ull : 0ull);
}
__device__ __forceinline__ int key_dist(unsigned long long k) { return (int)(k >> 41); }
__device__ __forceinline__ int key_idx(unsigned long long k) { return (int)((k >> 5) & 0xffffffull); }
__device__ __forceinline__ int key_octave(unsigned long long k) { return (int)((k >> 1) & 15ull); }
__device__ __forceinline__ bool key_held(unsigned long long k) { return (k & 1ull) != 0; }

// The words one pass of the claim iteration hands to the next - writer records, lists, results, flags - are written and read by
// DIFFERENT workgroups, but of DIFFERENT launches: a pass reads what the previous launch wrote (its own L1 starts empty) and
// writes what the next launch reads, never a word it also reads.  Plain loads and stores therefore do (rounds 3 - 4 kept them
// agent-scope atomics, sc1, for the sake of the persistent single-launch form, deleted in round 5): a record is two 16-byte
// loads that the L1 may keep for the other points of the CU that look at the same keypoint, a clear is 16-byte stores.  Only the
// read-modify-writes are atomics (record positions, list heads, the "changed" flag).
__device__ __forceinline__ int shared_load(const int *p) { return *p; }
__device__ __forceinline__ void shared_store(int *p, int v) { *p = v; }

// Writer table of a pass: per keypoint a 32-byte record {last position handed out, 7 entries}, entry = (4 * point + write
// kind) << 1 | (Observations() of the point > 0), -1 = empty; an eighth and later writer of one keypoint (never seen outside
// directed tests) goes to the overflow lists head / next, which hold the same entries.  One 32-byte read tells a later
// pass everything about a keypoint - where the linked lists of rounds 1-3 cost a dependent load per writer plus one for the
// writer's Observations() (a later pass is nothing but a chain of such round trips, ~1 us each).
#define FT_TAB_ENTRIES 7
// F.mvpMapPoints[kp] && ->Observations() > 0 as seen by map point i: the last writer j < i of the previous pass decides,
// else the pre-call holder (heldBefore)
struct LockRec {
    unsigned long long a, b, c, d;
};
__device__ __forceinline__ LockRec lock_record(const FtClaims &C, int kp) {
    const uint4 *rec = (const uint4 *)(C.tab + 8 * (size_t)kp);
    const uint4 lo = rec[0], hi = rec[1];
    LockRec r;
    r.a = (unsigned long long)lo.x | ((unsigned long long)lo.y << 32);
    r.b = (unsigned long long)lo.z | ((unsigned long long)lo.w << 32);
    r.c = (unsigned long long)hi.x | ((unsigned long long)hi.y << 32);
    r.d = (unsigned long long)hi.z | ((unsigned long long)hi.w << 32);
    return r;
}
// the decision of is_locked on a record that is already in registers (not a first pass)
__device__ __forceinline__ bool locked_by(const FtClaims &C, const LockRec &r, int kp, int i, bool heldBefore) {
    const unsigned long long a = r.a, b = r.b, c = r.c, d = r.d;
    const int last = (int)(unsigned)a;
    int best = -1;
    auto take = [&](int e) {
        if (e >= 0 && (e >> 3) < i && e > best) best = e;
    };
    take((int)(a >> 32)); take((int)(unsigned)b); take((int)(b >> 32)); take((int)(unsigned)c);
    take((int)(c >> 32)); take((int)(unsigned)d); take((int)(d >> 32));
    if (last >= FT_TAB_ENTRIES)
        for (int e = shared_load(&C.head[kp]); e >= 0; e = shared_load(&C.next[e >> 1])) take(e);
    return best >= 0 ? (best & 1) != 0 : heldBefore;
}
__device__ __forceinline__ bool is_locked(const FtClaims &C, int kp, int i, bool heldBefore) {
    if (C.firstPass) return heldBefore;
    return locked_by(C, lock_record(C, kp), kp, i, heldBefore);
}

// start of a claim-iteration pass (see FtClaims): false = the iteration has converged, nothing to do
// (blk of nblk: this workgroup among the frame's - the launch's own numbers unless the launcher laid the frames out itself)
__device__ __forceinline__ bool claims_begin_pass(const FtClaims &C, int blk, int nblk) {
    if (C.flagPrev && shared_load(C.flagPrev) == -1) {
        // batch form, first pass of a later burst: the frame had converged before this burst began.  Its flag words of this
        // burst's parity still hold what an earlier burst left there ("changed" for the passes it ran then): they all read
        // "unchanged" from here on, so that every later pass of the burst returns here as well.
        if (C.flagStick && blk == 0 && threadIdx.x < FT_BATCH_FLAGS / 2) shared_store(C.flagStick + threadIdx.x, -1);
        return false;
    }
    const int t = blk * blockDim.x + threadIdx.x, T = nblk * blockDim.x;
    for (int k = t; k < C.nKp; k += T) shared_store(&C.headClear[k], -1);
    uint4 *tc = (uint4 *)C.tabClear;  // (32-byte records, 32-byte aligned)
    for (int k = t; k < 2 * C.nKp; k += T) tc[k] = make_uint4(~0u, ~0u, ~0u, ~0u);
    if (t == 0) {
        shared_store(C.flagReset, -1);
        if (C.firstPass) shared_store(C.flagCur, 0);  // the first pass always "changes" its input
    }
    return true;
}
__device__ __forceinline__ bool claims_begin_pass(const FtClaims &C) { return claims_begin_pass(C, (int)blockIdx.x, (int)gridDim.x); }

// ---- B frames per launch (ft_tracked_batch) --------------------------------------------------------------------------------
// One frame at a time leaves the chip idle by construction: a pass of the claim iteration is ~500 workgroups and a handful
// of dependent L2 round trips, 9 - 13 passes per search, each a launch.  Here blockIdx.y is the FRAME: everything a pass
// needs of a frame - the frame itself, its points, its rotating claim buffers - sits in a job record in HBM (read through
// scalar loads: the address is uniform), the pass number selects the buffers exactly as fixedPoint (search_host.h) does for a
// launch of its own, and every frame has its own convergence flags, so that the workgroups of a frame whose iteration has
// reached its fixed point return at once while the other frames go on: the batch runs max-over-frames passes.
__device__ __forceinline__ FtClaims job_claims(const FtBatchJob &J, const Rebase &rb, int pass, int fCur, int fPrev, int fReset, int *&res) {
    const size_t K = (size_t)J.K, R = (size_t)4 * J.nPoints;
    int *head = rb(J.head), *tab = rb(J.tab), *next = rb(J.next), *resB = rb(J.res), *flags = rb(J.flags);
    FtClaims C;
    C.firstPass = pass == 0;
    C.head = head + (size_t)(pass % 3) * K;
    C.headWrite = head + (size_t)((pass + 1) % 3) * K;
    C.headClear = head + (size_t)((pass + 2) % 3) * K;
    C.tab = tab + (size_t)(pass % 3) * 8 * K;
    C.tabWrite = tab + (size_t)((pass + 1) % 3) * 8 * K;
    C.tabClear = tab + (size_t)((pass + 2) % 3) * 8 * K;
    C.next = next + (size_t)((pass + 1) & 1) * R;
    C.nextWrite = next + (size_t)(pass & 1) * R;
    C.resPrev = resB + (size_t)((pass + 1) & 1) * R;
    C.obs = rb(J.obs);
    C.nKp = J.nKp;
    C.flagCur = flags + fCur;
    C.flagPrev = fPrev >= 0 ? flags + fPrev : nullptr;
    C.flagReset = flags + fReset;
    C.flagStick = (fPrev >= 0 && (fPrev / (FT_BATCH_FLAGS / 2)) != (fCur / (FT_BATCH_FLAGS / 2))) ? flags + (fCur & ~(FT_BATCH_FLAGS / 2 - 1)) : nullptr;
    C.cache = rb(J.cache);
    res = resB + (size_t)(pass & 1) * R;
    return C;
}

__device__ __forceinline__ unsigned div_magic_u(int d) { return d > 1 ? 0xffffffffu / (unsigned)d + 1u : 0u; }

// key joins the two smallest keys seen (k0 <= k1), as selects: written as `if (key < k0) { k1 = k0; k0 = key; } else if
// (key < k1) k1 = key;` inside the window lambda the compiler selects between the ADDRESSES of k0 and k1 and keeps both in
// scratch memory - a load and a store per candidate
__device__ __forceinline__ void two_min_insert(unsigned long long &k0, unsigned long long &k1, unsigned long long key) {
    const unsigned long long larger = key < k0 ? k0 : key;
    k0 = key < k0 ? key : k0;
    k1 = larger < k1 ? larger : k1;
}

// ---- candidate cache of the claim iteration (FtClaims::cache): the meta word of a list ----
// (the lists are filed by the first pass that reaches a (point, camera) window: cache_append / cache_end in kernels_search.hip,
// row_cache_append / row_cache_end in kernels_search_rows.hip)
// The best candidates first.  A later pass needs the smallest (two smallest) UNLOCKED keys of a list, and a key's order is
// its distance before anything else: with the keys of the FT_CACHE_HEAD (or a few more) smallest distances at the front of
// the list, a pass that finds enough unlocked keys among them need not look at the rest - at th 15 a window holds ~190
// candidates, and every candidate looked at is a 32-byte record read.  A kernel of its own does it once behind the first pass
// of a batch (k_cache_partition_batch; inside the search kernels it cost them 45 registers): the smallest distance D with at
// least FT_CACHE_HEAD keys <= D by bisection over the 9 bits of the distance (a count per step), then a stable partition of
// the list by dist <= D.  The head's length goes into the meta word; a list that is short, or whose head would not be short
// (many equal distances), keeps head = count - as every list of the single-frame path does.
#ifndef FT_CACHE_HEAD
#define FT_CACHE_HEAD 16
#endif
#ifndef FT_CACHE_HEAD_MAX
#define FT_CACHE_HEAD_MAX 48
#endif
// length of the list's head (cache_partition): <= the count
__device__ __forceinline__ int cache_head(unsigned long long meta) { return (int)((meta >> 40) & 0x3ffull); }
// 0 = not built yet, 1 = usable (count = candidates filed), 2 = built but too many candidates: scan the window again
__device__ __forceinline__ int cache_state_of(unsigned long long meta, int &count, bool &anyInBox) {
    count = 0;
    anyInBox = false;
    if (meta == KEY_NONE) return 0;
    count = (int)(unsigned)meta;
    anyInBox = ((meta >> 32) & 1ull) != 0;
    return count <= FT_CACHE_CAP ? 1 : 2;
}

// A keypoint of a window as the scans see it: position, octave, uright, descriptor - from the search records of the grid
// (one 16-byte and one 32-byte read at the entry's position) or, without a grid, from the frame's own arrays.
struct WinEntry {
    float x, y, uright;  // uright: < 0 = none (or a two-camera frame)
    int idx, octave, cx, cy;
    unsigned long long d[4];
};
// level band and box test of GetFeaturesInArea for a keypoint whose cell is already known to lie in the window
__device__ __forceinline__ bool in_box(const WinEntry &kp, float x, float y, float r, int minLevel, int maxLevel) {
    const bool checkLevels = (minLevel > 0) || (maxLevel >= 0);
    if (checkLevels) {
        if (kp.octave < minLevel) return false;
        if (maxLevel >= 0 && kp.octave > maxLevel) return false;
    }
    const float dx = __fsub_rn(kp.x, x), dy = __fsub_rn(kp.y, y);
    return fabsf(dx) < r && fabsf(dy) < r;
}

// camera models: src/CameraModels/Pinhole.cpp:43-49, KannalaBrandt8.cpp:67-84
__device__ __forceinline__ void project_cam(const FtDevFrame &F, const float p[3], float uv[2]) {
    if (F.camModel == 0) {
        uv[0] = __fadd_rn(__fdiv_rn(__fmul_rn(F.cam[0], p[0]), p[2]), F.cam[2]);
        uv[1] = __fadd_rn(__fdiv_rn(__fmul_rn(F.cam[1], p[1]), p[2]), F.cam[3]);
    } else {
        const float x2y2 = __fadd_rn(__fmul_rn(p[0], p[0]), __fmul_rn(p[1], p[1]));
        const float theta = ft_atan2_f(sqrtf(x2y2), p[2]);
        const float psi = ft_atan2_f(p[1], p[0]);
        const float t2 = __fmul_rn(theta, theta);
        const float t3 = __fmul_rn(theta, t2);
        const float t5 = __fmul_rn(t3, t2);
        const float t7 = __fmul_rn(t5, t2);
        const float t9 = __fmul_rn(t7, t2);
        const float r = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(theta, __fmul_rn(F.cam[4], t3)), __fmul_rn(F.cam[5], t5)),
                                            __fmul_rn(F.cam[6], t7)),
                                  __fmul_rn(F.cam[7], t9));
        uv[0] = __fadd_rn(__fmul_rn(__fmul_rn(F.cam[0], r), ft_cos_f(psi)), F.cam[2]);
        uv[1] = __fadd_rn(__fmul_rn(__fmul_rn(F.cam[1], r), ft_sin_f(psi)), F.cam[3]);
    }
}


// The keypoints of camera `cam` whose grid cell lies in window w and whose octave lies in the level band of the search,
// handed to fn(entry) lane-parallel.  The frame's grid (k_build_grid) is a CSR PER OCTAVE: the keypoints of octave o in the
// cells (cx, minCY .. maxCY) are one contiguous range of entries - a map point looks at the keypoints GetFeaturesInArea would
// return for it (window AND level band: the band keeps 13 - 40 % of a window's keypoints, least where the windows are
// largest), where a grid over all octaves made the first pass of a search read every keypoint of the window.  Without a grid
// every keypoint's cell is computed and tested.
// minLevel / maxLevel as Frame::GetFeaturesInArea takes them (src/Frame.cc:714-729): no check at all unless minLevel > 0 or
// maxLevel >= 0; maxLevel < 0 = no upper bound.
template <class Fn>
__device__ __forceinline__ void for_window(const FtDevFrame &F, const FramePtrs &Q, int cam, const ft_keypoint *keys, int n, const Window &w,
                                           int minLevel, int maxLevel, int lane, Fn fn) {
    if (Q.gridStart[cam]) {
        // One lane per (octave, column of cells) range, a wave scan lays the ranges end to end, and the lanes take the
        // entries 64 at a time - two rounds per trip: record and descriptor of an entry sit at the entry's position, so a
        // round is one memory round trip, and a wide window a chain of them.
        const bool checkLevels = (minLevel > 0) || (maxLevel >= 0);
        const int lo = checkLevels ? min(max(minLevel, 0), F.nlevels - 1) : 0;  // (octaves beyond the table are filed under its last bucket)
        const int hi = (checkLevels && maxLevel >= 0) ? min(maxLevel, F.nlevels - 1) : F.nlevels - 1;
        const int ncolsW = w.maxCX - w.minCX + 1;
        const int npairs = (hi - lo + 1) * ncolsW;  // (<= 0: an empty band)
        const int *gs = Q.gridStart[cam];
        const float4 *rec = Q.gridRec[cam];
        const uint4 *gd = (const uint4 *)Q.gridDesc[cam];
        const unsigned colMagic = div_magic_u(ncolsW);
        for (int p0 = 0; p0 < npairs; p0 += 64) {
            const int np = min(64, npairs - p0);
            int b = 0, cnt = 0, myCol = 0;
            if (lane < np) {
                const int pidx = p0 + lane;
                const int oi = colMagic ? (int)__umulhi((unsigned)pidx, colMagic) : pidx;
                myCol = w.minCX + (pidx - oi * ncolsW);
                const int *col = gs + (size_t)(lo + oi) * (FT_GRID_CELLS + 1) + myCol * FT_GRID_ROWS;
                b = col[w.minCY];
                cnt = col[w.maxCY + 1] - b;
            }
            int incl = cnt;  // inclusive scan over the lanes
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(incl, d);
                if (lane >= d) incl += y;
            }
            const int total = __builtin_amdgcn_readlane(incl, 63);
            auto locate = [&](int t, int &pos, int &cx) {
                int r = 0;  // the range entry t falls into: the number of ranges that end at or before t
                for (int c = 0; c < np - 1; c++) r += t >= __builtin_amdgcn_readlane(incl, c) ? 1 : 0;
                const int cb = __shfl(b, r), cEnd = __shfl(incl, r), cCnt = __shfl(cnt, r);
                cx = __shfl(myCol, r);
                pos = cb + (t - (cEnd - cCnt));
            };
            auto hand = [&](const float4 &r, const uint4 &d0, const uint4 &d1, int cx) {
                WinEntry e;
                e.x = r.x; e.y = r.y; e.uright = r.z;
                const int io = __float_as_int(r.w);
                e.idx = io & 0xffffff;
                e.octave = io >> 24;  // (signed: the keypoint's own octave, whatever bucket it was filed under)
                e.cx = cx;
                e.cy = (int)roundf(__fmul_rn(__fsub_rn(r.y, F.mnMinY), F.invH));  // Frame::PosInGrid, as k_build_grid filed it
                e.d[0] = (unsigned long long)d0.x | ((unsigned long long)d0.y << 32);
                e.d[1] = (unsigned long long)d0.z | ((unsigned long long)d0.w << 32);
                e.d[2] = (unsigned long long)d1.x | ((unsigned long long)d1.y << 32);
                e.d[3] = (unsigned long long)d1.z | ((unsigned long long)d1.w << 32);
                fn(e);
            };
            for (int t0 = 0; t0 < total; t0 += 128) {
                const int tA = t0 + lane, tB = t0 + 64 + lane;
                int posA, cxA, posB = 0, cxB = 0;
                locate(min(tA, total - 1), posA, cxA);
                const bool second = t0 + 64 < total;  // wave-uniform
                if (second) locate(min(tB, total - 1), posB, cxB);
                const float4 rA = rec[posA];
                const uint4 a0 = gd[2 * (size_t)posA], a1 = gd[2 * (size_t)posA + 1];
                float4 rB = rA;
                uint4 b0 = a0, b1 = a1;
                if (second) {
                    rB = rec[posB];
                    b0 = gd[2 * (size_t)posB];
                    b1 = gd[2 * (size_t)posB + 1];
                }
                if (tA < total) hand(rA, a0, a1, cxA);
                if (second && tB < total) hand(rB, b0, b1, cxB);
            }
        }
        return;
    }
    const uint8_t *desc = Q.desc + (cam == 0 ? 0 : (size_t)F.Nleft * 32);
    for (int idx = lane; idx < n; idx += 64) {
        const ft_keypoint kp = keys[idx];
        const int cx = (int)roundf(__fmul_rn(__fsub_rn(kp.x, F.mnMinX), F.invW));
        const int cy = (int)roundf(__fmul_rn(__fsub_rn(kp.y, F.mnMinY), F.invH));
        if (cx < 0 || cx >= FT_GRID_COLS || cy < 0 || cy >= FT_GRID_ROWS) continue;  // never entered the grid
        if (cx < w.minCX || cx > w.maxCX || cy < w.minCY || cy > w.maxCY) continue;
        WinEntry e;
        e.x = kp.x; e.y = kp.y;
        e.uright = (cam == 0 && F.Nleft == -1 && Q.uright) ? Q.uright[idx] : -1.0f;
        e.idx = idx; e.octave = kp.octave; e.cx = cx; e.cy = cy;
        const unsigned long long *dp = (const unsigned long long *)(desc + (size_t)idx * 32);
        e.d[0] = dp[0]; e.d[1] = dp[1]; e.d[2] = dp[2]; e.d[3] = dp[3];
        fn(e);
    }
}

// ---- poses and distances (the float chains of the reference, every operation rounded on its own) ----
__device__ __forceinline__ void transform34(const float *T, const float x[3], float y[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++)
        y[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4 * r], x[0]), __fmul_rn(T[4 * r + 1], x[1])),
                                   __fmul_rn(T[4 * r + 2], x[2])),
                         T[4 * r + 3]);
}

// Sophus::SE3f * point as the reference's CPU branch evaluates `Tcw * x3Dw` (src/ORBmatcher.cc:1805) and `GetRelativePoseTrl() *
// x3Dc` (:1900): Thirdparty/Sophus/sophus/so3.hpp:358-367 - uv = q.vec().cross(p); uv += uv; p + q.w() * uv + q.vec().cross(uv) -
// then + translation (se3.hpp:321-324); every product and sum rounded on its own, coefficient order as Eigen's cross()
__device__ __forceinline__ void cross3_rn(const float a[3], const float b[3], float c[3]) {
    c[0] = __fsub_rn(__fmul_rn(a[1], b[2]), __fmul_rn(a[2], b[1]));
    c[1] = __fsub_rn(__fmul_rn(a[2], b[0]), __fmul_rn(a[0], b[2]));
    c[2] = __fsub_rn(__fmul_rn(a[0], b[1]), __fmul_rn(a[1], b[0]));
}
__device__ __forceinline__ void transform_pose(const float *m, const float *q, int quat, const float x[3], float y[3]) {
    if (!quat) {
        transform34(m, x, y);
        return;
    }
    float uv[3], c[3];
    cross3_rn(q, x, uv);
#pragma unroll
    for (int i = 0; i < 3; i++) uv[i] = __fadd_rn(uv[i], uv[i]);
    cross3_rn(q, uv, c);
#pragma unroll
    for (int i = 0; i < 3; i++) y[i] = __fadd_rn(__fadd_rn(__fadd_rn(x[i], __fmul_rn(q[3], uv[i])), c[i]), m[4 * i + 3]);
}

// Eigen's sum of three terms (dot, squaredNorm, a coefficient of a small matrix product): redux_novec_unroller splits the
// range in halves, e0 + (e1 + e2) (see the oracle's note at orc_is_in_frustum)
__device__ __forceinline__ float dot3(const float *a, const float *b) {
    return __fadd_rn(__fmul_rn(a[0], b[0]), __fadd_rn(__fmul_rn(a[1], b[1]), __fmul_rn(a[2], b[2])));
}
// sqrtf is correctly rounded here (-fhip-fp32-correctly-rounded-divide-sqrt); __fsqrt_rn maps to the native approximation
__device__ __forceinline__ float norm3(const float *a) { return sqrtf(dot3(a, a)); }

__device__ __forceinline__ int predict_scale(float maxDistanceRaw, float dist, float logScaleFactor, int nLevels) {
    const float ratio = __fdiv_rn(maxDistanceRaw, dist);
    const float lg = ft_libm::logf_glibc(ratio);
    int nScale = (int)ceilf(__fdiv_rn(lg, logScaleFactor));
    if (nScale < 0) nScale = 0;
    else if (nScale >= nLevels) nScale = nLevels - 1;
    return nScale;
}

// key joins the ascending t[0 .. N): the N smallest candidate keys of a lane (kernels_reloc.hip, kernels_sim3.hip)
template <int N>
__device__ __forceinline__ void top_insert(unsigned long long t[N], unsigned long long key) {
#pragma unroll
    for (int k = 0; k < N; k++) {
        const unsigned long long lo = key < t[k] ? key : t[k];
        key = key < t[k] ? t[k] : key;
        t[k] = lo;
    }
}

// ---- the grid of a frame (k_build_grid, k_build_grid_batch: kernels_frame.hip; k_fuse_grid: kernels_fuse.hip) ----
// Frame::AssignFeaturesToGrid (src/Frame.cc:409-440) as one CSR per octave: workgroup (octave o, camera) counting-sorts the
// camera's keypoints of octave o by cell cx * 48 + cy in LDS and files them behind the keypoints of the lower octaves (their
// number is counted on the way).  An octave outside [0, nlevels) is filed under the nearest bucket; the searches test the
// keypoint's own octave anyway.  The order inside a cell is free (the searches order candidates by (distance, cx, cy, index)
// keys).  start: [nlevels][FT_GRID_CELLS + 1] absolute entry positions; rec / desc: the entries (ft_search.h).
__device__ __forceinline__ void build_grid_body(const FtDevFrame &F, const FramePtrs &Q, int oct, int cam, int *startL, int *startR,
                                                float4 *recL, uint8_t *descL, float4 *recR, uint8_t *descR) {
    __shared__ int cnt[FT_GRID_CELLS + 1];
    __shared__ int wsum[4], wbelow[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = cam == 0 ? (F.Nleft == -1 ? F.N : F.Nleft) : (F.Nleft == -1 ? 0 : F.N - F.Nleft);
    const ft_keypoint *keys = cam == 0 ? Q.keys : Q.keysR;
    int *start = (cam == 0 ? startL : startR);
    if (!start) return;
    start += (size_t)oct * (FT_GRID_CELLS + 1);
    for (int c = tid; c <= FT_GRID_CELLS; c += 256) cnt[c] = 0;
    __syncthreads();
    auto cellOf = [&](const ft_keypoint &kp) -> int {
        const int cx = (int)roundf(__fmul_rn(__fsub_rn(kp.x, F.mnMinX), F.invW));
        const int cy = (int)roundf(__fmul_rn(__fsub_rn(kp.y, F.mnMinY), F.invH));
        if (cx < 0 || cx >= FT_GRID_COLS || cy < 0 || cy >= FT_GRID_ROWS) return -1;
        return cx * FT_GRID_ROWS + cy;
    };
    int below = 0;  // keypoints of the grid in lower buckets
    for (int i = tid; i < n; i += 256) {
        const ft_keypoint kp = keys[i];
        const int c = cellOf(kp);
        if (c < 0) continue;
        const int bkt = min(max(kp.octave, 0), F.nlevels - 1);
        if (bkt < oct) below++;
        else if (bkt == oct) atomicAdd(&cnt[c], 1);
    }
    below = wave_sum_i32(below);
    if (lane == 0) wbelow[wave] = below;
    __syncthreads();
    // exclusive scan of the 3072 counts: 12 consecutive cells per thread
    constexpr int PER = FT_GRID_CELLS / 256;
    int local = 0;
    for (int k = 0; k < PER; k++) local += cnt[tid * PER + k];
    int incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    const int base = wbelow[0] + wbelow[1] + wbelow[2] + wbelow[3];
    int run = base + incl - local;
    for (int w = 0; w < wave; w++) run += wsum[w];
    const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    for (int k = 0; k < PER; k++) {
        const int c = tid * PER + k, v = cnt[c];
        start[c] = run;
        cnt[c] = run;  // becomes the fill cursor of the cell
        run += v;
    }
    if (tid == 0) start[FT_GRID_CELLS] = base + total;
    __syncthreads();
    float4 *rec = cam == 0 ? recL : recR;
    uint8_t *gdesc = cam == 0 ? descL : descR;
    const uint8_t *desc = Q.desc + (cam == 0 ? 0 : (size_t)F.Nleft * 32);
    for (int i = tid; i < n; i += 256) {
        const ft_keypoint kp = keys[i];
        const int c = cellOf(kp);
        if (c < 0 || min(max(kp.octave, 0), F.nlevels - 1) != oct) continue;
        const int p = atomicAdd(&cnt[c], 1);
        const float ur = (cam == 0 && F.Nleft == -1 && Q.uright) ? Q.uright[i] : -1.0f;
        rec[p] = make_float4(kp.x, kp.y, ur, __int_as_float((i & 0xffffff) | (kp.octave << 24)));
        const uint4 *d = (const uint4 *)(desc + (size_t)i * 32);
        uint4 *o = (uint4 *)(gdesc + (size_t)p * 32);
        o[0] = d[0];
        o[1] = d[1];
    }
}

// ---- a map point as a ROW of 16 lanes (kernels_search_rows.hip, kernels_fuse.hip) ----
__device__ __forceinline__ int row_shfl(int v, int srcLane) { return __shfl(v, srcLane); }
// The window scan of a row's point, in three steps through a small LDS list of the row (FT_ROW_LIST entries; the lanes of a row
// belong to one wave, whose LDS operations are served in order - no barrier):
//   expand  a lane per (octave, column of cells) range, a DPP scan lays the ranges end to end, and every range lane writes the
//           grid positions of its entries (with the column in the top byte) at their places in the list - where the first form of
//           this loop looked the range of every entry up again, 16 entries at a time, by a chain of np - 1 shuffles;
//   filter  16 entries at a time: the 16-byte record, level band and box test of GetFeaturesInArea (in_box), the survivors packed
//           to the front of the list by a ballot of the row - the cell ranges of a window hold ~2.4 x the keypoints of the box, and
//           the other 58 % leave here without their descriptor having been loaded;
//   visit   fn(entry, real) for the survivors, 16 at a time: descriptor, cell row, and whatever the search does with them.
// Windows with more entries than the list holds go through it in parts.  What fn sees is what it saw before minus the entries
// in_box rejects (the order inside a list is free).
#define FT_ROW_LIST 64
__device__ __forceinline__ void row_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
template <class Fn>
__device__ __forceinline__ void row_for_window(const FtDevFrame &F, const FramePtrs &Q, int cam, const Window &w, int minLevel, int maxLevel,
                                               float bx, float by, float br, int sub, int rowBase, unsigned *list, Fn fn) {
    const bool checkLevels = (minLevel > 0) || (maxLevel >= 0);
    const int lo = checkLevels ? min(max(minLevel, 0), F.nlevels - 1) : 0;
    const int hi = (checkLevels && maxLevel >= 0) ? min(maxLevel, F.nlevels - 1) : F.nlevels - 1;
    const int ncolsW = w.maxCX - w.minCX + 1;
    const int npairs = (hi - lo + 1) * ncolsW;  // (<= 0: an empty band)
    const int *gs = Q.gridStart[cam];
    const float4 *rec = Q.gridRec[cam];
    const uint4 *gd = (const uint4 *)Q.gridDesc[cam];
    const unsigned colMagic = div_magic_u(ncolsW);
    for (int p0 = 0; p0 < npairs; p0 += 16) {  // (row-uniform)
        const int np = min(16, npairs - p0);
        int b = 0, cnt = 0, myCol = 0;
        if (sub < np) {
            const int pidx = p0 + sub;
            const int oi = colMagic ? (int)__umulhi((unsigned)pidx, colMagic) : pidx;
            myCol = w.minCX + (pidx - oi * ncolsW);
            const int *col = gs + (size_t)(lo + oi) * (FT_GRID_CELLS + 1) + myCol * FT_GRID_ROWS;
            b = col[w.minCY];
            cnt = col[w.maxCY + 1] - b;
        }
        int incl = cnt;  // inclusive scan over the 16 lanes of the row (lanes shifted in from outside the row read 0)
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, true);  // row_shr:1
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, true);  // row_shr:2
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, true);  // row_shr:4
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, true);  // row_shr:8
        const int total = row_shfl(incl, rowBase + 15);
        const int start = incl - cnt;
        const unsigned tag = (unsigned)b | ((unsigned)myCol << 24);  // (grid positions stay below 2^24, columns below 64)
        for (int w0 = 0; w0 < total; w0 += FT_ROW_LIST) {  // (row-uniform)
            const int nw = min(FT_ROW_LIST, total - w0);
            // expand: the part of this lane's range that falls into [w0, w0 + nw)
            for (int k = max(0, w0 - start), k1 = min(cnt, w0 + nw - start); k < k1; k++) list[start + k - w0] = tag + (unsigned)k;
            row_lds_sync();
            // filter: survivors of the box to the front (an entry is read before its group writes, and a group writes below its
            // own first entry + 16)
            int m = 0;
            for (int t0 = 0; t0 < nw; t0 += 16) {  // (row-uniform)
                const int t = t0 + sub;
                const unsigned v = list[min(t, nw - 1)];
                const float4 rr = rec[v & 0xffffffu];
                WinEntry e;
                e.x = rr.x; e.y = rr.y;
                e.octave = __float_as_int(rr.w) >> 24;
                const bool inb = t < nw && in_box(e, bx, by, br, minLevel, maxLevel);
                const unsigned bits = (unsigned)(__ballot(inb) >> rowBase) & 0xffffu;
                if (inb) list[m + __popc(bits & ((1u << sub) - 1u))] = v;
                m += __popc(bits);
            }
            row_lds_sync();
            // visit
            for (int s0 = 0; s0 < m; s0 += 16) {  // (row-uniform)
                const int sI = s0 + sub;
                const unsigned v = list[min(sI, m - 1)];
                const int pos = (int)(v & 0xffffffu);
                const float4 rr = rec[pos];
                const uint4 d0 = gd[2 * (size_t)pos], d1 = gd[2 * (size_t)pos + 1];
                WinEntry e;
                e.x = rr.x; e.y = rr.y; e.uright = rr.z;
                const int io = __float_as_int(rr.w);
                e.idx = io & 0xffffff;
                e.octave = io >> 24;
                e.cx = (int)(v >> 24);
                e.cy = (int)roundf(__fmul_rn(__fsub_rn(rr.y, F.mnMinY), F.invH));
                e.d[0] = (unsigned long long)d0.x | ((unsigned long long)d0.y << 32);
                e.d[1] = (unsigned long long)d0.z | ((unsigned long long)d0.w << 32);
                e.d[2] = (unsigned long long)d1.x | ((unsigned long long)d1.y << 32);
                e.d[3] = (unsigned long long)d1.z | ((unsigned long long)d1.w << 32);
                fn(e, sI < m);
            }
            row_lds_sync();  // (the next part - or the next window - overwrites the list)
        }
    }
}

}  // namespace

// Host side of the projection searches, shared by the translation units of the entry-point families (search_view.cpp,
// tracked_frame.cpp, init_search.cpp, reloc_search.cpp, triang_search.cpp and newpoints.cpp (through triang_host.h), fuse_search.cpp, sim3_search.cpp, tracked_batch.cpp; bow.cpp, bow_kf_search.cpp,
// distinct_desc.cpp and fisheye_match.cpp for the call skeleton at the end: CallScope, over the Arena of fv_host.h): replaces launchSearchLocalPointsKernel / launchPoseEstimationKernel
// (reference include/Kernels/KernelController.h:40-46) together with the acceptance loops the reference keeps in the caller
// (src/ORBmatcher.cc:241-308, 2013-2081).  Windowing, level/box tests and every Hamming distance run on the device
// (kernels_search*.hip, kernels_resolve.hip, kernels_frame.hip); the host only marshals arrays, drives the fixed-point passes and
// replays the O(M) write list in map point order to produce mvpMapPoints / the rotation histogram, exactly as the reference's caller does.
// Host only: no kernel includes this header.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "ft_host.h"
#include "ft_search.h"
#include "fv_host.h"
#include "rot_hist.h"

// One ft_bow_side in the arena of a SearchByBoW call (bow.cpp, beside checkBowSide): the FeatureVector, then what the call stages of
// the side - has: its has_point, desc: its descriptors (not those of a frame that are resident on the device), angles: its
// keypoint angles (check_orientation).  The FeatureVector comes first, so offset 0 = "not in the arena".
struct BowSideLayout {
    FvLayout fv;
    size_t desc, hasPoint, angles;
};
BowSideLayout layoutBowSide(Arena &a, const ft_bow_side *s, bool has, bool desc, bool angles);
// fills the arena's pinned mirror; the record says nLeft = -1, nUn = n (a side without a second camera)
FtBowArenaSide stageBowSide(const ft_bow_side *s, const uint8_t *has, const BowSideLayout &L, uint8_t *pin);

struct FrameLayout {
    size_t keys, keysR, desc, uright, holder, l2r, r2l;
    int nLeftKeys, nRightKeys;
};

inline int checkFrame(const ft_frame_view *F) {
    FT_REQUIRE(F, "null frame view");
    FT_REQUIRE(F->N >= 0 && F->N < (1 << 24), "frame keypoint count out of range");
    FT_REQUIRE(F->Nleft == -1 || (F->Nleft >= 0 && F->Nleft <= F->N), "Nleft out of range");
    FT_REQUIRE(F->N == 0 || (F->keys && F->descriptors && F->holder_obs), "frame arrays are null");
    FT_REQUIRE(F->Nleft == -1 || F->N == F->Nleft || F->keys_right, "keys_right is null");
    FT_REQUIRE(F->Nleft == -1 || (F->left_to_right && F->right_to_left), "stereo match tables are null");
    FT_REQUIRE(F->scale_factors && F->nlevels >= 1 && F->nlevels <= FT_MAX_LEVELS, "scale factors missing");
    FT_REQUIRE(F->cam_model == 0 || F->cam_model == 1, "unknown camera model");
    // the searches read a keypoint's octave back from four bits of a candidate key (make_key, search_dev.h)
    const int nL = F->Nleft == -1 ? F->N : F->Nleft, nR = F->Nleft == -1 ? 0 : F->N - F->Nleft;
    for (int i = 0; i < nL; i++) FT_REQUIRE(F->keys[i].octave >= 0 && F->keys[i].octave < F->nlevels, "keypoint octave outside [0, nlevels)");
    for (int i = 0; i < nR; i++)
        FT_REQUIRE(F->keys_right[i].octave >= 0 && F->keys_right[i].octave < F->nlevels, "right keypoint octave outside [0, nlevels)");
    return FT_OK;
}

inline void layoutFrame(const ft_frame_view *F, Arena &a, FrameLayout &L) {
    L.nLeftKeys = F->Nleft == -1 ? F->N : F->Nleft;
    L.nRightKeys = F->Nleft == -1 ? 0 : F->N - F->Nleft;
    L.keys = a.take(sizeof(ft_keypoint) * std::max(L.nLeftKeys, 1));
    L.keysR = a.take(sizeof(ft_keypoint) * std::max(L.nRightKeys, 1));
    L.desc = a.take((size_t)32 * std::max(F->N, 1));
    L.uright = a.take(sizeof(float) * std::max(F->N, 1));
    L.holder = a.take(sizeof(int) * std::max(F->N, 1));
    L.l2r = a.take(sizeof(int) * std::max(L.nLeftKeys, 1));
    L.r2l = a.take(sizeof(int) * std::max(L.nRightKeys, 1));
}

inline void stageFrame(const ft_frame_view *F, const FrameLayout &L, uint8_t *pin) {
    if (L.nLeftKeys) memcpy(pin + L.keys, F->keys, sizeof(ft_keypoint) * L.nLeftKeys);
    if (L.nRightKeys) memcpy(pin + L.keysR, F->keys_right, sizeof(ft_keypoint) * L.nRightKeys);
    if (F->N) memcpy(pin + L.desc, F->descriptors, (size_t)32 * F->N);
    if (F->uright && F->N) memcpy(pin + L.uright, F->uright, sizeof(float) * F->N);
    if (F->N) memcpy(pin + L.holder, F->holder_obs, sizeof(int) * F->N);
    if (F->Nleft != -1) {
        if (L.nLeftKeys) memcpy(pin + L.l2r, F->left_to_right, sizeof(int) * L.nLeftKeys);
        if (L.nRightKeys) memcpy(pin + L.r2l, F->right_to_left, sizeof(int) * L.nRightKeys);
    }
}

// frame constants of a view (no arrays)
inline FtDevFrame devFrameConstants(const ft_frame_view *F) {
    FtDevFrame D;
    memset(&D, 0, sizeof D);
    D.N = F->N;
    D.Nleft = F->Nleft;
    D.mnMinX = F->mnMinX; D.mnMinY = F->mnMinY; D.mnMaxX = F->mnMaxX; D.mnMaxY = F->mnMaxY;
    D.invW = F->grid_inv_w; D.invH = F->grid_inv_h;
    D.mbf = F->mbf; D.mb = F->mb;
    D.camModel = F->cam_model;
    memcpy(D.cam, F->cam, sizeof D.cam);
    memcpy(D.Trl, F->Trl, sizeof D.Trl);
    for (int i = 0; i < F->nlevels && i < FT_MAX_LEVELS; i++) D.sf[i] = F->scale_factors ? F->scale_factors[i] : 1.f;
    D.nlevels = F->nlevels;
    return D;
}

inline FtDevFrame devFrame(const ft_frame_view *F, const FrameLayout &L, uint8_t *dev) {
    FtDevFrame D = devFrameConstants(F);
    D.keys = (const ft_keypoint *)(dev + L.keys);
    D.keysR = (const ft_keypoint *)(dev + L.keysR);
    D.desc = dev + L.desc;
    D.uright = F->uright ? (const float *)(dev + L.uright) : nullptr;
    D.holderObs = (const int *)(dev + L.holder);
    D.l2r = F->Nleft != -1 ? (const int *)(dev + L.l2r) : nullptr;
    D.r2l = F->Nleft != -1 ? (const int *)(dev + L.r2l) : nullptr;
    return D;
}

// Runs `search` passes until a pass changes nothing; the final results are on the host (through `download`) when it returns.
// A pass is ONE launch: the search kernel files every point's writes in the writer lists the next pass reads (three rotating
// head arrays: read / write / clear) and flags any change against the previous pass's results.  Passes are enqueued in
// bursts of FT_PASS_BURST without waiting in between; a pass first looks at the previous pass's flag and returns at once
// when the fixed point has been reached (it would reproduce its input), so the surplus passes of a burst cost an empty
// launch each while every avoided round trip (D2H of the flags + stream sync) costs ~100 us.  One memset (0xff: list heads
// = -1, flags = "unchanged") prepares a call.
#define FT_PASS_BURST_MAX 14  // flag slots per burst parity (16) and the 64-byte flag window of the pinned result area bound it
// passes per burst: with the candidate cache a pass is ~12 us and an early-exit pass ~5 us, a round trip to the host ~40 us,
// and a search needs 9 - 13 passes - one burst of 12 mostly does it (FT_PASS_BURST=<n> to experiment)
inline int passBurst(const ft_context *ctx) { return std::min(std::max(ctx->tuning.pass_burst, 2), FT_PASS_BURST_MAX); }
// device buffers of the claim iteration: res 2 x 4 nPoints ints, head 3 x nKp directly followed by 16 flag ints (two burst
// parities x FT_PASS_BURST), next 2 x 4 nPoints
struct PassBufs {
    int *res, *head, *next;
    const int *obs;
    unsigned long long *cache;  // FT_CACHE_WORDS per point, or null (FT_SEARCH_CACHE=0)
};
// `download(res, flags, nFlagBytes)` enqueues ONE delivery kernel that writes the pass results `res`, whatever else the
// caller needs and the burst's flags into pinned host memory (hostFlags); it runs behind every burst, in front of the one
// stream synchronisation.
template <typename SearchFn, typename DownloadFn>
inline int fixedPoint(ft_context *ctx, hipStream_t st, int nPoints, int nKp, const PassBufs &B, FtClaims &C, SearchFn search,
               DownloadFn download, const int *hostFlags, int **resFinal, int *passes, int *burstHint = nullptr) {
    // Passes per burst.  Every surplus pass of a burst is an empty launch (4.5 us of dispatch for ~500 workgroups), every
    // burst that falls short a host round trip (~40 us).  A caller that searches frame after frame (ft_tracked_frame) hands in
    // the pass count of its previous search of the same kind: the first burst is that count + 1, later bursts are short.
    // Without a hint: option pass_burst (12) for every burst.
    const int burstMax = passBurst(ctx);
    int FT_PASS_BURST = burstHint && *burstHint > 0 ? std::min(std::max(*burstHint + 1, 4), FT_PASS_BURST_MAX) : burstMax;
    *resFinal = B.res;
    *passes = 0;
    if (nPoints <= 0) {
        int rc0 = download(B.res, nullptr, 0);
        if (rc0 != FT_OK) return rc0;
        FT_HIP(hipStreamSynchronize(st));
        return FT_OK;
    }
    const size_t K = ((size_t)std::max(nKp, 1) + 7) & ~(size_t)7;  // = passK(nKp)
    int *flags = B.head + 3 * K, *tab = flags + 32;  // (the table records are 32 bytes and 32-byte aligned: layoutPasses)
    const int fillWords = (int)(3 * K + 32 + 24 * K);
    {   // list heads = -1, flags = "unchanged" (-1), writer table empty (-1); candidate cache: ~0 in a slot's first word = "not built yet"
        const int rcf = ft_launch_fill_claims(st, B.head, fillWords, B.cache, 2 * nPoints, FT_CACHE_CAP + 1);
        if (rcf != FT_OK) return rcf;
    }
    C.cache = B.cache;
    int pass = 0, burst = 0;
    const int maxPasses = 2 * nPoints + 4 + burstMax;
    C.obs = B.obs;
    C.nKp = nKp;
    int *last = B.res;
    for (;; burst++) {
        int *fl = flags + 16 * (burst & 1), *flOther = flags + 16 * ((burst + 1) & 1);
        for (int b = 0; b < FT_PASS_BURST; b++, pass++) {
            C.firstPass = pass == 0;
            C.head = B.head + (size_t)(pass % 3) * K;
            C.headWrite = B.head + (size_t)((pass + 1) % 3) * K;
            C.headClear = B.head + (size_t)((pass + 2) % 3) * K;
            C.tab = tab + (size_t)(pass % 3) * 8 * K;
            C.tabWrite = tab + (size_t)((pass + 1) % 3) * 8 * K;
            C.tabClear = tab + (size_t)((pass + 2) % 3) * 8 * K;
            C.next = B.next + (size_t)((pass + 1) & 1) * 4 * nPoints;
            C.nextWrite = B.next + (size_t)(pass & 1) * 4 * nPoints;
            C.resPrev = B.res + (size_t)((pass + 1) & 1) * 4 * nPoints;
            C.flagCur = fl + b;
            C.flagPrev = b > 0 ? fl + b - 1 : nullptr;
            C.flagReset = flOther + b;
            last = B.res + (size_t)(pass & 1) * 4 * nPoints;
            const int rc = search(last);
            if (rc != FT_OK) return rc;
        }
        // after a converged burst both result buffers hold the fixed point (the last pass that ran reproduced its input)
        int rc = download(last, fl, sizeof(int) * FT_PASS_BURST);
        if (rc != FT_OK) return rc;
        FT_HIP(hipStreamSynchronize(st));
        const int *h = hostFlags;
        if (h[FT_PASS_BURST - 1] == -1) {  // the last pass of the burst changed nothing (or did not have to run)
            int ran = 0;
            while (ran < FT_PASS_BURST && h[ran] != -1) ran++;
            pass = pass - FT_PASS_BURST + std::min(ran + 1, FT_PASS_BURST);
            break;
        }
        if (pass >= maxPasses) {
            ft_set_error("projection search: claim resolution did not converge");
            return FT_ERR_HIP;
        }
        if (burstHint) FT_PASS_BURST = 4;  // the hint fell short: short bursts from here
    }
    *resFinal = last;
    *passes = pass;
    if (burstHint) *burstHint = pass;
    return FT_OK;
}

// arena space of the claim iteration for M points on a frame of N keypoints
struct PassLayout {
    size_t res, head, next, cache;
    bool haveCache;
};
// keypoint count of the claim buffers: a multiple of 8, so that the 32-byte table records behind 3 K heads + 32 flags are aligned
inline size_t passK(int N) { return ((size_t)std::max(N, 1) + 7) & ~(size_t)7; }
inline bool searchCacheOn(const ft_context *ctx) { return ctx->tuning.search_cache != 0; }
inline size_t searchCacheBytes(int M) { return 8 * (size_t)FT_CACHE_WORDS * (size_t)std::max(M, 1); }
// cacheInArena: the candidate cache (device only, 8 KB per point) lives at the end of the arena - the stand-alone searches,
// whose arena sizes the context's device scratch; a tracked frame owns a cache buffer of its own, so that its pinned mirror
// of the arena stays small
inline PassLayout layoutPasses(const ft_context *ctx, Arena &a, int M, int N, bool cacheInArena) {
    PassLayout L;
    L.res = a.take(32 * (size_t)M);
    L.head = a.take(4 * (3 * passK(N) + 32 + 24 * passK(N)));  // list heads, flags, writer table (fixedPoint)
    L.next = a.take(32 * (size_t)M);
    L.haveCache = cacheInArena && searchCacheOn(ctx);
    L.cache = L.haveCache ? a.take(searchCacheBytes(M)) : 0;
    return L;
}
inline PassBufs passBufs(const PassLayout &L, uint8_t *dev, const int *obs, unsigned long long *ownCache = nullptr) {
    PassBufs B;
    B.res = (int *)(dev + L.res);
    B.head = (int *)(dev + L.head);
    B.next = (int *)(dev + L.next);
    B.obs = obs;
    B.cache = L.haveCache ? (unsigned long long *)(dev + L.cache) : ownCache;
    return B;
}
// Frame::mGrid of a frame staged in the arena: CSR arrays behind the frame's own, built by one small launch
// cell starts per octave of both cameras (FT_MAX_LEVELS x 3073 ints each), then the entries as 16-byte search records and
// 32-byte descriptors
inline size_t gridIntBytes(int) { return (sizeof(int) * 2 * (size_t)FT_MAX_LEVELS * (FT_GRID_CELLS + 1) + 15) & ~(size_t)15; }
inline size_t gridBytes(int N) { return gridIntBytes(N) + 48 * (size_t)std::max(N, 1); }
inline size_t layoutGrid(Arena &a, int N) { return a.take(gridBytes(N)); }
// the grid arrays of frame DF inside `grid` (gridBytes(DF.N)): cell starts of both cameras, records, descriptors
inline void pointGrid(FtDevFrame &DF, int *grid) {
    const int nL = DF.Nleft == -1 ? DF.N : DF.Nleft;
    const bool two = DF.Nleft != -1;
    float4 *rec = (float4 *)((uint8_t *)grid + gridIntBytes(DF.N));
    uint8_t *gdesc = (uint8_t *)(rec + std::max(DF.N, 1));
    DF.gridStart[0] = grid;
    DF.gridStart[1] = two ? grid + (size_t)FT_MAX_LEVELS * (FT_GRID_CELLS + 1) : nullptr;
    DF.gridRec[0] = rec;
    DF.gridDesc[0] = gdesc;
    DF.gridRec[1] = two ? rec + nL : nullptr;
    DF.gridDesc[1] = two ? gdesc + (size_t)32 * nL : nullptr;
}
// one launch builds it (the frame's arrays are the memory the pointers name: the kernel writes through them)
inline int launchGrid(hipStream_t st, FtDevFrame &DF, int *grid) {
    FtDevFrame G = DF;
    pointGrid(G, grid);
    const int rc = ft_launch_build_grid(st, DF, (int *)G.gridStart[0], (int *)G.gridStart[1], (float4 *)G.gridRec[0], (uint8_t *)G.gridDesc[0],
                                        (float4 *)G.gridRec[1], (uint8_t *)G.gridDesc[1]);
    if (rc == FT_OK) DF = G;
    return rc;
}
// the projection searches' grid: where option search_grid asks for it
inline int buildGrid(const ft_context *ctx, hipStream_t st, FtDevFrame &DF, int *grid) {
    return ctx->tuning.search_grid ? launchGrid(st, DF, grid) : FT_OK;
}

// Replays the writes of SearchByProjection(Frame, points) in map point order (ORBmatcher.cc:134-148 left,
// :203-214 right): res holds per point the keypoints written as (primary left, side left, primary right, side right).
inline int replayLocalWrites(const int *res, int M, const int *observations, int *holder, int *assign) {
    int nm = 0;
    for (int i = 0; i < M; i++) {
        const int obs = observations[i];
        const int order[4] = {res[4 * i], res[4 * i + 1], res[4 * i + 3], res[4 * i + 2]};  // primL sideL sideR primR
        for (int k = 0; k < 4; k++) {
            const int kp = order[k];
            if (kp < 0) continue;
            holder[kp] = obs;
            assign[kp] = i;
            nm++;
        }
    }
    return nm;
}

// Replays the writes of SearchByProjection(CurrentFrame, LastFrame) in last-frame order with the rotation histogram
// of ORBmatcher.cc:1880-1896, 1942-1957, 1966-1987 and ComputeThreeMaxima (:2210-2251): rot_hist.h.  curAngle(i) = angle of
// keypoint i of the current frame (left keypoints, then right).
template <typename AngleFn>
inline int replayLastFrameWrites(const int *res, int M, const ft_last_points *L, AngleFn curAngle, bool checkOrientation, int *holder,
                          int *assign) {
    int nm = 0;
    RotHist hist;
    for (int i = 0; i < M; i++) {
        const int w2[2] = {res[4 * i], res[4 * i + 2]};
        for (int k = 0; k < 2; k++) {
            const int kp = w2[k];
            if (kp < 0) continue;
            holder[kp] = L->observations[i];
            assign[kp] = i;
            nm++;
            if (checkOrientation) hist.add(L->angle[i], curAngle(kp), kp);
        }
    }
    hist.forDropped([&](int kp) { assign[kp] = holder[kp] = -1, nm--; });
    return nm;
}

// camera poses of isInFrustumChecks (Frame.cc:1312-1325); compiled without contraction, sums associated as Eigen does
inline FtFrustumPose frustumPose(const ft_frame_view *F, const ft_frame_pose *T) {
    FtFrustumPose P;
    memcpy(P.R[0], T->Rcw, sizeof P.R[0]);
    memcpy(P.t[0], T->tcw, sizeof P.t[0]);
    memcpy(P.twc[0], T->Ow, sizeof P.twc[0]);
    const float *Trl = F->Trl;
    auto sum3 = [](float e0, float e1, float e2) { return e0 + (e1 + e2); };  // Eigen's association (redux_novec_unroller)
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++)
            P.R[1][3 * i + j] = sum3(Trl[4 * i] * T->Rcw[j], Trl[4 * i + 1] * T->Rcw[3 + j], Trl[4 * i + 2] * T->Rcw[6 + j]);
        P.t[1][i] = sum3(Trl[4 * i] * T->tcw[0], Trl[4 * i + 1] * T->tcw[1], Trl[4 * i + 2] * T->tcw[2]) + Trl[4 * i + 3];
        P.twc[1][i] = sum3(T->Rcw[i] * T->tlr[0], T->Rcw[3 + i] * T->tlr[1], T->Rcw[6 + i] * T->tlr[2]) + T->Ow[i];
    }
    return P;
}

inline FtFrustumPose frustumPose_fromDev(const FtDevFrame &DF, const ft_frame_pose *T) {
    ft_frame_view v;
    memset(&v, 0, sizeof v);
    memcpy(v.Trl, DF.Trl, sizeof v.Trl);
    return frustumPose(&v, T);
}

inline int checkMapPoints(const ft_map_points *P, bool forSearch) {
    FT_REQUIRE(P && P->M >= 0 && P->M < (1 << 22), "map point count out of range");
    FT_REQUIRE(P->M == 0 || (P->world_pos && P->normal && P->max_distance && P->min_distance), "map point arrays are null");
    FT_REQUIRE(!forSearch || P->M == 0 || (P->descriptors && P->observations), "map point descriptors / observations are null");
    return FT_OK;
}

struct FrustumLayout {
    size_t skip, pos, nrm, maxd, mind;                                      // inputs
    size_t inV, inVR, lvl, lvlR, vc, vcR, px, py, pxr, pyr, dep, depR, sskip, count;  // outputs
};

inline void layoutFrustum(int M, bool hasSkip, Arena &a, FrustumLayout &L, size_t *inputEnd) {
    const size_t m = (size_t)std::max(M, 1);
    L.skip = a.take(hasSkip ? m : 1);
    L.pos = a.take(12 * m);
    L.nrm = a.take(12 * m);
    L.maxd = a.take(4 * m);
    L.mind = a.take(4 * m);
    *inputEnd = a.off;
    L.inV = a.take(m); L.inVR = a.take(m);
    L.lvl = a.take(4 * m); L.lvlR = a.take(4 * m);
    L.vc = a.take(4 * m); L.vcR = a.take(4 * m);
    L.px = a.take(4 * m); L.py = a.take(4 * m); L.pxr = a.take(4 * m); L.pyr = a.take(4 * m);
    L.dep = a.take(4 * m); L.depR = a.take(4 * m);
    L.sskip = a.take(m);
    L.count = a.take(64);
}

inline void stageFrustum(const ft_map_points *P, const FrustumLayout &L, uint8_t *pin) {
    const size_t M = (size_t)P->M;
    if (!M) return;
    if (P->skip) memcpy(pin + L.skip, P->skip, M);
    memcpy(pin + L.pos, P->world_pos, 12 * M);
    memcpy(pin + L.nrm, P->normal, 12 * M);
    memcpy(pin + L.maxd, P->max_distance, 4 * M);
    memcpy(pin + L.mind, P->min_distance, 4 * M);
}

inline FtDevMapPoints devMapPoints(const ft_map_points *P, const FrustumLayout &L, uint8_t *dev) {
    FtDevMapPoints D;
    D.M = P->M;
    D.skip = P->skip ? dev + L.skip : nullptr;
    D.worldPos = (const float *)(dev + L.pos);
    D.normal = (const float *)(dev + L.nrm);
    D.maxDist = (const float *)(dev + L.maxd);
    D.minDist = (const float *)(dev + L.mind);
    return D;
}

inline FtFrustumOut devFrustumOut(const FrustumLayout &L, uint8_t *dev) {
    FtFrustumOut O;
    O.inView = dev + L.inV; O.inViewR = dev + L.inVR;
    O.level = (int *)(dev + L.lvl); O.levelR = (int *)(dev + L.lvlR);
    O.viewCos = (float *)(dev + L.vc); O.viewCosR = (float *)(dev + L.vcR);
    O.projX = (float *)(dev + L.px); O.projY = (float *)(dev + L.py);
    O.projXR = (float *)(dev + L.pxr); O.projYR = (float *)(dev + L.pyr);
    O.depth = (float *)(dev + L.dep); O.depthR = (float *)(dev + L.depR);
    O.searchSkip = dev + L.sskip;
    O.count = (int *)(dev + L.count);
    return O;
}

// the frustum fields of the output block [outBegin, ...) that sits at the start of `pin`
inline void unpackFrustum(int M, const FrustumLayout &L, size_t outBegin, uint8_t *pin, const ft_frustum_result *R, int *n_to_match) {
    auto at = [&](size_t off) { return pin + (off - outBegin); };
    if (n_to_match) *n_to_match = *(const int *)at(L.count);
    if (!R || !M) return;
    const size_t m = (size_t)M;
    if (R->in_view) memcpy(R->in_view, at(L.inV), m);
    if (R->in_view_r) memcpy(R->in_view_r, at(L.inVR), m);
    if (R->level) memcpy(R->level, at(L.lvl), 4 * m);
    if (R->level_r) memcpy(R->level_r, at(L.lvlR), 4 * m);
    if (R->view_cos) memcpy(R->view_cos, at(L.vc), 4 * m);
    if (R->view_cos_r) memcpy(R->view_cos_r, at(L.vcR), 4 * m);
    if (R->proj_x) memcpy(R->proj_x, at(L.px), 4 * m);
    if (R->proj_y) memcpy(R->proj_y, at(L.py), 4 * m);
    if (R->proj_xr) memcpy(R->proj_xr, at(L.pxr), 4 * m);
    if (R->proj_yr) memcpy(R->proj_yr, at(L.pyr), 4 * m);
    if (R->depth) memcpy(R->depth, at(L.dep), 4 * m);
    if (R->depth_r) memcpy(R->depth_r, at(L.depR), 4 * m);
}
// D2H of the frustum fields the caller asked for (one contiguous copy of the output block, then scatter)
inline int downloadFrustum(hipStream_t st, int M, const FrustumLayout &L, size_t outBegin, size_t outEnd, uint8_t *dev, uint8_t *pin,
                    const ft_frustum_result *R, int *n_to_match) {
    FT_HIP(hipMemcpyAsync(pin, dev + outBegin, outEnd - outBegin, hipMemcpyDeviceToHost, st));
    FT_HIP(hipStreamSynchronize(st));
    unpackFrustum(M, L, outBegin, pin, R, n_to_match);
    return FT_OK;
}

inline FtPose poseOfMatrix(const float *T) {
    FtPose p;
    memset(&p, 0, sizeof p);
    memcpy(p.m, T, sizeof p.m);
    return p;
}
inline int poseOfSe3(const ft_se3 *T, FtPose &p) {
    memset(&p, 0, sizeof p);
    const float n2 = T->q[0] * T->q[0] + T->q[1] * T->q[1] + T->q[2] * T->q[2] + T->q[3] * T->q[3];
    if (!(n2 > 0.99f && n2 < 1.01f)) {
        ft_set_error("ft_se3: q is not a unit quaternion (x, y, z, w)");
        return FT_ERR_INVALID;
    }
    p.m[0] = p.m[5] = p.m[10] = 1.f;
    p.m[3] = T->t[0]; p.m[7] = T->t[1]; p.m[11] = T->t[2];
    memcpy(p.q, T->q, sizeof p.q);
    p.quat = 1;
    return FT_OK;
}
// the right camera's pose of a frame in the Sophus form, in place of the matrix of its view
inline void setTrl(FtDevFrame &DF, const FtPose &trl) {
    memcpy(DF.Trl, trl.m, sizeof DF.Trl);
    memcpy(DF.TrlQ, trl.q, sizeof DF.TrlQ);
    DF.trlQuat = trl.quat;
}

// Tcw (and Trl, which a two-camera frame must bring) of an _se3 entry point `what`; *trlPtr = &trl or null
inline int posesFromSe3(const ft_se3 *Tcw, const ft_se3 *Trl, bool twoCamera, const char *what, FtPose &pose, FtPose &trl,
                        const FtPose **trlPtr) {
    if (!Trl && twoCamera) {
        ft_set_error(std::string(what) + ": a two-camera frame needs Trl");
        return FT_ERR_INVALID;
    }
    int rc = poseOfSe3(Tcw, pose);
    if (rc == FT_OK && Trl) rc = poseOfSe3(Trl, trl);
    *trlPtr = Trl ? &trl : nullptr;
    return rc;
}

// The points of SearchByProjection(CurrentFrame, LastFrame): count (capacity < 0: the library's own limit, else that of the
// `owner` - "frame" / "batch" - the call belongs to) and arrays; with nlevels > 0 also the octaves of the valid points.  The
// entry points ask twice: without the octaves in front of their default outputs, with them once there is something to search
// (a batch that reads the arrays in place leaves the octaves to the device).
inline int checkLastPoints(const ft_last_points *L, int nlevels, int capacity, const char *owner) {
    const int M = L->N;
    if (capacity < 0) FT_REQUIRE(M >= 0 && M < (1 << 22), "last-frame point count out of range");
    else FT_REQUIRE(M >= 0 && M <= capacity, std::string("last-frame point count beyond the ") + owner + "'s capacity");
    FT_REQUIRE(M == 0 || (L->valid && L->world_pos && L->descriptors && L->observations && L->octave && L->angle),
               "last-frame arrays are null");
    for (int i = 0; i < M && nlevels > 0; i++)
        FT_REQUIRE(!L->valid[i] || (L->octave[i] >= 0 && L->octave[i] < nlevels), "last-frame octave out of range");
    return FT_OK;
}

struct LastLayout {
    size_t valid, pos, desc, obs, oct;
};
inline LastLayout layoutLast(Arena &a, size_t M) {
    LastLayout L;
    L.valid = a.take(M);
    L.pos = a.take(12 * M);
    L.desc = a.take(32 * M);
    L.obs = a.take(4 * M);
    L.oct = a.take(4 * M);
    return L;
}
inline void stageLast(const ft_last_points *P, const LastLayout &L, uint8_t *pin) {
    const size_t M = (size_t)P->N;
    if (!M) return;
    memcpy(pin + L.valid, P->valid, M);
    memcpy(pin + L.pos, P->world_pos, 12 * M);
    memcpy(pin + L.desc, P->descriptors, 32 * M);
    memcpy(pin + L.obs, P->observations, 4 * M);
    memcpy(pin + L.oct, P->octave, 4 * M);
}
inline FtDevLastPoints devLast(int M, const LastLayout &L, uint8_t *dev) {
    FtDevLastPoints D;
    D.N = M;
    D.valid = dev + L.valid;
    D.worldPos = (const float *)(dev + L.pos);
    D.desc = dev + L.desc;
    D.octave = (const int *)(dev + L.oct);
    D.angle = nullptr;
    return D;
}

// The map points of ORBmatcher::Fuse and of SearchByProjection(pKF, Scw, ...): `who` is the entry point with its job, "name: "
inline int checkPoints(const ft_fuse_points &P, const std::string &who) {
    FT_REQUIRE(P.M >= 0 && P.M < (1 << 22), who + "map point count out of range");
    FT_REQUIRE(P.M == 0 || (P.world_pos && P.normal && P.max_distance && P.min_distance && P.descriptors), who + "map point arrays are null");
    return FT_OK;
}
struct PointsLayout {
    size_t pos, nrm, maxd, mind, desc;
};
inline PointsLayout layoutPoints(Arena &a, size_t M) {
    PointsLayout L;
    L.pos = a.take(12 * M);
    L.nrm = a.take(12 * M);
    L.maxd = a.take(4 * M);
    L.mind = a.take(4 * M);
    L.desc = a.take(32 * M);
    return L;
}
inline void stagePoints(const ft_fuse_points *P, const PointsLayout &L, uint8_t *pin) {
    const size_t M = (size_t)P->M;
    if (!M) return;
    memcpy(pin + L.pos, P->world_pos, 12 * M);
    memcpy(pin + L.nrm, P->normal, 12 * M);
    memcpy(pin + L.maxd, P->max_distance, 4 * M);
    memcpy(pin + L.mind, P->min_distance, 4 * M);
    memcpy(pin + L.desc, P->descriptors, 32 * M);
}
inline FtFusePoints devPoints(int M, const PointsLayout &L, uint8_t *dev) {
    FtFusePoints D;
    D.M = M;
    D.worldPos = (const float *)(dev + L.pos);
    D.normal = (const float *)(dev + L.nrm);
    D.maxDist = (const float *)(dev + L.maxd);
    D.minDist = (const float *)(dev + L.mind);
    D.desc = dev + L.desc;
    return D;
}

// One camera of a keyframe as the one-camera frame those two searches scan: n keypoints `keys` with descriptor rows `desc`
struct FuseSide {
    int n, idxOffset;  // idxOffset: NLeft for the right camera
    const ft_keypoint *keys;
    const uint8_t *desc;
    const float *uright;  // mvuRight where the keyframe has it (one camera), else null
};
inline int checkKeyframeSide(const ft_frame_view *F, bool right, const std::string &who, FuseSide &s) {
    FT_REQUIRE(F, who + "null keyframe view");
    FT_REQUIRE(F->N >= 0 && F->N < (1 << 24), who + "keypoint count out of range");
    FT_REQUIRE(F->Nleft == -1 || (F->Nleft >= 0 && F->Nleft <= F->N), who + "Nleft out of range");
    FT_REQUIRE(!right || F->Nleft != -1, who + "right on a keyframe with one camera (Nleft == -1)");
    FT_REQUIRE(F->cam_model == 0 || F->cam_model == 1, who + "unknown camera model");
    FT_REQUIRE(F->scale_factors && F->nlevels >= 1 && F->nlevels <= FT_MAX_LEVELS, who + "scale factors missing");
    if (right) {
        s.n = F->N - F->Nleft;
        s.idxOffset = F->Nleft;
        s.keys = F->keys_right;
        s.desc = F->descriptors ? F->descriptors + (size_t)32 * F->Nleft : nullptr;
        s.uright = nullptr;
    } else {
        s.n = F->Nleft == -1 ? F->N : F->Nleft;
        s.idxOffset = 0;
        s.keys = F->keys;
        s.desc = F->descriptors;
        s.uright = F->Nleft == -1 ? F->uright : nullptr;
    }
    FT_REQUIRE(s.n == 0 || (s.keys && s.desc), who + "keypoints or descriptors are null");
    // the search reads a keypoint's octave back from four bits of its key (make_key, search_dev.h) and indexes inv_level_sigma2 with it
    for (int i = 0; i < s.n; i++) FT_REQUIRE(s.keys[i].octave >= 0 && s.keys[i].octave < F->nlevels, who + "keypoint octave outside [0, nlevels)");
    return FT_OK;
}
// the grid of that camera: cell starts per octave, then the entries as 16-byte records and 32-byte descriptors (ft_search.h)
inline size_t sideStartBytes(int nlevels) { return (sizeof(int) * (size_t)nlevels * (FT_GRID_CELLS + 1) + 63) & ~(size_t)63; }
inline size_t sideGridBytes(int nlevels, int n) { return sideStartBytes(nlevels) + 48 * (size_t)std::max(n, 1); }
inline void pointSideGrid(FtDevFrame &F, uint8_t *grid, int nlevels, int n) {
    float4 *rec = (float4 *)(grid + sideStartBytes(nlevels));
    F.gridStart[0] = (const int *)grid;
    F.gridRec[0] = rec;
    F.gridDesc[0] = (const uint8_t *)(rec + std::max(n, 1));
}

// the frustum outputs as the inputs of SearchByProjection(Frame, points), where they are on the device
inline FtDevLocalPoints localPointsOf(const FtFrustumOut &O, int M, const uint8_t *desc) {
    FtDevLocalPoints P;
    P.M = M;
    P.skip = O.searchSkip; P.inView = O.inView; P.inViewR = O.inViewR;
    P.level = O.level; P.levelR = O.levelR;
    P.viewCos = O.viewCos; P.viewCosR = O.viewCosR;
    P.projX = O.projX; P.projY = O.projY; P.projXR = O.projXR; P.projYR = O.projYR;
    P.desc = desc;
    return P;
}

// a block the delivery kernel of a search takes down to pinned memory together with the pass results
struct DeliverAlong {
    void *dst = nullptr;
    const void *src = nullptr;
    size_t bytes = 0;
};

// The claim passes of one single-frame search (fixedPoint) with their delivery: the results (16 bytes per point) to hRes
// (pinned) with the burst's 64-byte flag window behind them, `along` in the same launch.
template <typename SearchFn>
int runPasses(ft_context *ctx, int nPoints, int nKp, const PassBufs &B, FtClaims &C, SearchFn search, uint8_t *hRes,
              const DeliverAlong &along, int *passes, int *burstHint) {
    hipStream_t st = ctx->stream;
    const size_t resBytes = 16 * (size_t)nPoints;
    int *resFinal = nullptr;
    return fixedPoint(ctx, st, nPoints, nKp, B, C, search,
                      [&](int *res, const int *fl, size_t flBytes) -> int {
                          return ft_launch_deliver_blocks(st, hRes, res, resBytes, along.dst, along.src, along.bytes, hRes + resBytes, fl, flBytes);
                      },
                      (const int *)(hRes + resBytes), &resFinal, passes, burstHint);
}

// The two single-frame searches behind their staging: the claim passes of the points on the device frame DF, then the replay
// of their writes into holder / assign (*nm matches, *passes claim passes).  B: the claim buffers (B.obs: the points'
// observations on the device); rawDev: device block of the raw best-distance arrays (k x M ints in the order of FtLastRaw /
// FtLocalRaw) or null; burstHint: fixedPoint's or null; hRes, along: runPasses'.
template <typename AngleFn>
int runLastFrameSearch(ft_context *ctx, const FtDevFrame &DF, const FtDevLastPoints &DL, const PassBufs &B, int *rawDev, int *burstHint,
                       const FtPose &pose, float th, int forward, int backward, uint8_t *hRes, const DeliverAlong &along,
                       const ft_last_points *L, bool checkOrientation, AngleFn curAngle, int *holder, int *assign, int *nm, int *passes) {
    auto rawAt = [&](int k) { return rawDev ? rawDev + (size_t)k * DL.N : nullptr; };
    const FtLastRaw raw = {rawAt(0), rawAt(1), rawAt(2), rawAt(3)};
    FtClaims C;
    const int rc = runPasses(ctx, DL.N, DF.N, B, C,
                             [&](int *res) { return ft_launch_search_last(ctx->stream, DF, DL, C, pose, th, forward, backward, res, raw); },
                             hRes, along, passes, burstHint);
    if (rc != FT_OK) return rc;
    *nm = replayLastFrameWrites((const int *)hRes, DL.N, L, curAngle, checkOrientation, holder, assign);
    return FT_OK;
}

inline int runLocalSearch(ft_context *ctx, const FtDevFrame &DF, const FtDevLocalPoints &DP, const PassBufs &B, int *rawDev, int *burstHint,
                          float th, float nn_ratio, uint8_t *hRes, const DeliverAlong &along, const int *observations, int *holder,
                          int *assign, int *nm, int *passes) {
    auto rawAt = [&](int k) { return rawDev ? rawDev + (size_t)k * DP.M : nullptr; };
    const FtLocalRaw raw = {rawAt(0), rawAt(1), rawAt(2), rawAt(3), rawAt(4), rawAt(5), rawAt(6), rawAt(7), rawAt(8), rawAt(9)};
    FtClaims C;
    const int rc = runPasses(ctx, DP.M, DF.N, B, C, [&](int *res) { return ft_launch_search_local(ctx->stream, DF, DP, C, th, nn_ratio, res, raw); },
                             hRes, along, passes, burstHint);
    if (rc != FT_OK) return rc;
    *nm = replayLocalWrites((const int *)hRes, DP.M, observations, holder, assign);
    return FT_OK;
}

// Device-resident frame (ft_tracked_frame_*): owns (or borrows from a stereo front end) the keypoint / descriptor
// arrays in HBM; the scalar part of the frame, the host copy of the keypoints (angles for the rotation histogram)
// and the authoritative holder_obs live on the host and are cheap (a few KB per frame).
struct ft_tracked_frame {
    unsigned long long *d_cache = nullptr;  // candidate cache of the claim iteration (FtClaims::cache), maxPts points
    bool counted = false;  // registered with the context (ft_context::liveObjects)
    ft_context *ctx = nullptr;
    int maxKp = 0, maxPts = 0;
    // owned device storage
    ft_keypoint *d_keys = nullptr, *d_keysR = nullptr;
    uint8_t *d_desc = nullptr;
    float *d_uright = nullptr;
    int *d_holder = nullptr, *d_l2r = nullptr, *d_r2l = nullptr;
    int *d_grid = nullptr;                         // Frame::mGrid as CSR (both cameras), built when a frame is loaded
    uint8_t *d_work = nullptr, *h_work = nullptr;  // per-call arena (points, passes, outputs) and its pinned mirror
    int *h_holderUp = nullptr;                       // pinned source of the holder_obs uploads (see uploadHolder)
    uint8_t *h_frameUp = nullptr;                    // pinned staging of ft_tracked_frame_upload (all arrays of a frame)
    size_t frameUpBytes = 0;
    size_t workBytes = 0;
    // current frame
    bool loaded = false;
    FtDevFrame DF;
    std::vector<float> angles;  // angle of keypoint i (left then right)
    std::vector<int> holder;
    int passesLast = 0, passesLocal = 0;  // claim passes of the previous search of each kind: the next one's burst size (fixedPoint)
    // ORBmatcher::SearchForInitialization with this frame as the current one (runInitSearch): keypoints of octave 0, and the
    // call's arena with its pinned mirror (grow-only; the candidate segments are level0 x level0 words of two frames).  The
    // relocalisation search (reloc_search.cpp) takes its arena from the same pair: both hold nothing between calls.
    int level0 = 0;
    uint8_t *d_init = nullptr, *h_init = nullptr;
    size_t initDevBytes = 0, initPinBytes = 0;
    FtEventTimer evt;
};

// The grow-only arena of a tracked frame's one-shot searches (d_init / h_init): a stream of frames settles after a few calls
inline int ensureInitArena(ft_tracked_frame *tf, size_t devBytes, size_t pinBytes) {
    if (devBytes <= tf->initDevBytes && pinBytes <= tf->initPinBytes) return FT_OK;
    FT_HIP(hipStreamSynchronize(tf->ctx->stream));
    if (tf->d_init) hipFree(tf->d_init);
    if (tf->h_init) hipHostFree(tf->h_init);
    tf->d_init = tf->h_init = nullptr;
    tf->initDevBytes = tf->initPinBytes = 0;
    FT_HIP(hipMalloc((void **)&tf->d_init, devBytes + devBytes / 4));
    tf->initDevBytes = devBytes + devBytes / 4;
    FT_HIP(hipHostMalloc((void **)&tf->h_init, pinBytes + pinBytes / 4, hipHostMallocDefault));
    tf->initPinBytes = pinBytes + pinBytes / 4;
    return FT_OK;
}

// ---- a one-shot call on an arena and its pinned mirror: the keyframe matchers, bow.cpp, fisheye_match.cpp's fisheye / distance calls, search_view.cpp's queries ----
// The event timer of a stand-alone call, destroyed with the call's scope.  (FtEventTimer itself has no destructor: extractors,
// tracked frames and batches keep theirs for their lifetime and destroy it where they free their streams.)
struct CallEventTimer {
    FtEventTimer evt;
    ~CallEventTimer() { evt.destroy(); }
};
// What such a call enqueues on the context's stream between its arena `dev` and the arena's pinned mirror `pin` (the context's
// scratch, or a tracked frame's own arena with the frame's timer): blocks up, launches, one block down - and one wait.  The first
// failure sticks: what follows is skipped, and down() waits for what was enqueued before the error leaves the entry point (the
// next call may free the arena).  Every path of an entry point behind its first up() ends in down() (ft_features_in_area: per phase).
struct CallScope {
    ft_context *ctx;
    hipStream_t st;
    uint8_t *dev, *pin;
    FtEventTimer &evt;
    int launches = 0;
    int rc = FT_OK;
    void hip(hipError_t e, const char *what) {
        if (e != hipSuccess && rc == FT_OK) rc = ft_hip_fail(e, what, __FILE__, __LINE__);
    }
    void up(size_t begin, size_t end) {
        if (rc == FT_OK) hip(hipMemcpyAsync(dev + begin, pin + begin, end - begin, hipMemcpyHostToDevice, st), "hipMemcpyAsync (block up)");
    }
    // an input the caller holds in pinned memory goes up from where it is (ft_is_pinned_host_range), not through the mirror
    void upFrom(size_t begin, const void *src, size_t bytes) {
        if (rc == FT_OK) hip(hipMemcpyAsync(dev + begin, src, bytes, hipMemcpyHostToDevice, st), "hipMemcpyAsync (block up)");
    }
    void zero(size_t begin, size_t end) {
        if (rc == FT_OK) hip(hipMemsetAsync(dev + begin, 0, end - begin, st), "hipMemsetAsync");
    }
    // fn() enqueues one kernel; name: its kernel.* stat under ft_context_set_kernel_timing, null = not timed
    template <typename Fn>
    void launch(const char *name, Fn fn) {
        if (rc != FT_OK) return;
        const bool tm = ctx->kernelTiming && name;
        evt.begin(tm, name, st);
        rc = fn();
        evt.end(tm, st);
        launches++;
    }
    // a block down without the wait, in front of down(): for outputs that come down cheaper apart than as one block (ft_bow_transform)
    void downBlock(size_t begin, size_t end) {
        if (rc == FT_OK) hip(hipMemcpyAsync(pin + begin, dev + begin, end - begin, hipMemcpyDeviceToHost, st), "hipMemcpyAsync (block down)");
    }
    int down(size_t begin, size_t end) {
        downBlock(begin, end);
        hip(hipStreamSynchronize(st), "hipStreamSynchronize");
        if (rc == FT_OK) evt.resolve(ctx);
        else evt.recs.clear(), evt.used = 0;
        return rc;
    }
};

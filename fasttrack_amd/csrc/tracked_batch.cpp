// B device-resident frames searched through ONE set of launches (ft_tracked_batch_*; SURVEY.md 7 step 7 "Batch API (B frames
// per launch)").  One frame at a time is what the reference's tracking thread does (src/Tracking.cc:2911-2989, 3472-3555) and it
// leaves a 256-CU chip idle by construction: ~45 launches of a few hundred workgroups per frame.  A batch holds B independent
// frames - the camera streams of one time step, or any frames whose inputs the caller has - and runs every stage as one launch
// over all of them: grid build (blockIdx.z = frame), isInFrustum, and each pass of the two searches' claim iteration
// (blockIdx.y = frame, per-frame convergence flags; the batch runs max-over-frames passes).  Results per frame are those of
// ft_tracked_frame_* on that frame, bit for bit.
//
// Memory: ONE device arena per batch (the kernels re-derive every pointer of a job record from it: Rebase, ft_search.h; FramePtrs, search_dev.h)
//   work   | per call: job records, delivery records, the frames' point arrays (compact), frustum outputs
//   frames | keypoints, descriptors, uright, match tables, holder_obs of the uploaded frames (compact)
//   flags  | 32 words per frame;  counts | 1 word per frame (isInFrustum's nToMatch)
//   grid   | Frame::mGrid as CSR, per frame;  claims | res, list heads + writer table, next, per frame;  cache | per frame
// and two pinned buffers: the mirror of `work` + `frames` (inputs: one H2D copy per call) and the results.
// One search of a batch between its two halves (submit: everything up to the first point where the host must look at the flag
// words, enqueued; wait: the rest).  Holds what the second half needs of the call: nothing of the caller's argument arrays is
// referenced after submit except the OUTPUT arrays, whose pointers are copied here.
#include "search_host.h"

struct FtBatchCall {
    int kind = 0;  // 0 = none in flight, 1 = SearchByProjection(CurrentFrame, LastFrame), 2 = isInFrustum + SearchByProjection(Frame, points)
    int n = 0, maxPoints = 0, maxK = 8, maxM = 0, maxFrWords = 0, shInts = 0;
    const FtBatchJob *dJobs = nullptr;
    const FtDeliverRec *dRecs = nullptr;
    float th = 0.f, nnRatio = 0.f, viewingCosLimit = 0.f, logScaleFactor = 0.f, thFar = 0.f;
    int farPoints = 0, checkOrientation = 0;
    bool useResolve = false, frustumDone = false;
    // the claim iteration, split where the host first waits for the device
    int pass = 0, burst = 0, len = 0, prevLen = 0, parity = 0, nextB = 0;
    bool simple = false, awaitResolve = false, resolvedAll = false;
    // results in tb->h_out
    size_t oFlagsOut = 0, oNmOut = 0, oCountsOut = 0, oErrOut = 0;
    std::vector<size_t> outAssign, outFr, fInEnd;
    std::vector<FrustumLayout> FL;
    std::vector<int> M;
    // the caller's output arrays
    std::vector<int *> assign;
    bool assignDirect = false;  // every assign[f] lies in pinned memory: k_replay_batch writes there, the wait copies nothing
    bool frustumDirect = false;  // every array of every frustum[f] lies in pinned memory: a scatter launch behind k_frustum_batch fills them
    const FtGatherRec *dFrRecs = nullptr;
    int nFrRecs = 0;
    int *nMatches = nullptr, *nToMatch = nullptr;
    std::vector<ft_frustum_result> frustum;
    bool haveFrustum = false;
    FtTimer tAll;
};

struct ft_tracked_batch {
    ft_context *ctx = nullptr;
    bool counted = false;
    int maxFrames = 0, maxKp = 0, maxPts = 0;
    uint8_t *d_arena = nullptr;
    size_t arenaBytes = 0;
    size_t oWork = 0, workBytes = 0, oFrames = 0, framesBytes = 0, oFlags = 0, oCounts = 0, oGrid = 0, gridStride = 0, oClaims = 0,
           claimStride = 0, oCache = 0, cacheStride = 0;
    uint8_t *h_in = nullptr;   // pinned mirror of [work | frames]
    uint8_t *h_out = nullptr;  // pinned results
    size_t outBytes = 0;
    // the uploaded frames
    int nFrames = 0;
    std::vector<FtDevFrame> DF;
    // holder_obs (Observations() of mvpMapPoints[i], -1 = none) lives in HBM from the upload on: the searches read it there and
    // k_replay_batch updates it there; ft_tracked_batch_holder_obs copies a frame's array down on request
    std::vector<size_t> holderOff;  // byte offset of frame f's holder_obs inside the frames region
    size_t holderBegin = 0, holderEnd = 0;  // the holder_obs arrays of all frames are contiguous: one copy takes them up
    size_t oReplayed = 0;  // one int per frame: k_replay_batch's "this search's writes have been replayed" marker
    int passesLast = 0, passesLocal = 0;
    bool hasGrid = false;  // the frames' CSR grids were laid out and built at upload / bind time (search_grid as it was THEN)
    // the context's search options as the current call saw them (snapshotTuning, under ctx->matchMutex): the option may be set
    // from another thread while a call runs, and a call must not see two values of it
    int optSearchCache = 0, optPassBurst = 0;
    // a stream and a lock of the batch's own: two batches of one context used from two host threads are two batches in flight -
    // the passes of one run beside the host side (staging, replay) of the other
    hipStream_t stream = nullptr;
    std::mutex mu;
    FtEventTimer evt;  // ft_context_set_kernel_timing: HIP events around the batch's launches on the context's stream
    hipEvent_t evGather = nullptr;  // bind_fisheye: the gather from the extractors' slots has run (the extractors' next batch waits for it)
    hipEvent_t evMirror = nullptr;  // the last copy out of the pinned mirror h_in has run: the next call may repack it
    FtBatchCall call;  // the search between ft_tracked_batch_submit_* and ft_tracked_batch_wait (kind 0: none)
    size_t oErr = 0;   // one int per frame: input errors the kernels found (a last-frame octave outside the frame's levels)
};

namespace {

size_t batchClaimBytes(int maxKp, int maxPts) {
    const size_t K = passK(maxKp);
    return ((32 * (size_t)maxPts + 63) & ~(size_t)63) * 2 + ((4 * 27 * K + 63) & ~(size_t)63) + 4 * (16 + 2 * (size_t)maxPts) + 64;
}
// bytes of one frame's arrays in the frames region, upper bound
size_t batchFrameBytes(int maxKp) {
    const size_t K = (size_t)maxKp;
    return (2 * sizeof(ft_keypoint) + 32 + 4 * 4) * K + 8 * 64;
}
// per call and frame: point inputs (<= 69 B), frustum outputs (<= 47 B) per point + alignment slack
size_t batchWorkBytes(int maxPts) { return 128 * (size_t)maxPts + 26 * 64 + sizeof(FtBatchJob) + 4 * sizeof(FtDeliverRec); }
size_t batchOutBytes(int maxPts) { return (16 + 47) * (size_t)maxPts + 20 * 64; }

// the claim buffers of frame f for a search of nPoints points on nKp keypoints
void batchClaims(const ft_tracked_batch *tb, int f, int nKp, int nPoints, FtBatchJob &J) {
    uint8_t *c = tb->d_arena + tb->oClaims + (size_t)f * tb->claimStride;
    const size_t resBytes = (32 * (size_t)tb->maxPts + 63) & ~(size_t)63;
    J.res = (int *)c;
    J.next = (int *)(c + resBytes);
    J.head = (int *)(c + 2 * resBytes);
    J.K = (int)passK(nKp);
    J.tab = J.head + 3 * (size_t)J.K;
    J.slow = (int *)(c + 2 * resBytes + ((4 * 27 * passK(tb->maxKp) + 63) & ~(size_t)63));
    J.flags = (int *)(tb->d_arena + tb->oFlags) + FT_BATCH_FLAGS * (size_t)f;
    J.cache = tb->oCache ? (unsigned long long *)(tb->d_arena + tb->oCache + (size_t)f * tb->cacheStride) : nullptr;
    J.nKp = nKp;
    J.nPoints = nPoints;
    J.replayed = (int *)(tb->d_arena + tb->oReplayed) + f;
    J.err = (int *)(tb->d_arena + tb->oErr) + f;
}

// first pass of a batched search by the four-points-per-wave kernels (k_search_*_first) where the cache and the grid exist (and
// under search_cache = 2 the rest of the search by k_resolve_batch)
#ifndef FT_ROW_FIRST
#define FT_ROW_FIRST 1
#endif
// search_cache 2: the one-launch resolution for batches of FT_RESOLVE_MIN_FRAMES frames and more.  Its chain is as long for one
// frame as for 256 (a workgroup per frame: 0.26 / 0.5 ms per search at configs[3]) while a claim pass over few frames is a
// 10-us launch: one batch alone is served sooner by the passes up to ~56 frames (1 frame 0.19 against 0.33 ms, 32 frames 0.57
// against 0.65), several batches in flight more cheaply by the resolution from ~24 on (32 frames x 4 lanes: 22.4 k against
// 17.4 k frames/s) - EXPERIMENTS 10.8.  search_cache 3: every batch.
#ifndef FT_RESOLVE_MIN_FRAMES
#define FT_RESOLVE_MIN_FRAMES 24
#endif
// (callers hold tb->mu) the options a batch call works with: read once per call under the mutex ft_context_set_option writes under
void snapshotTuning(ft_tracked_batch *tb) {
    std::lock_guard<std::mutex> lk(tb->ctx->matchMutex);
    tb->optSearchCache = tb->ctx->tuning.search_cache;
    tb->optPassBurst = std::min(std::max(tb->ctx->tuning.pass_burst, 2), FT_PASS_BURST_MAX);
}
bool resolveWanted(const ft_tracked_batch *tb, int nFrames) {
    const int sc = tb->optSearchCache;
    return sc >= 3 || (sc == 2 && nFrames >= FT_RESOLVE_MIN_FRAMES);
}
// the row-first kernels and the one-launch resolution read the candidate cache AND the frames' grids: both must have been laid out
// when the batch was created / the frames were uploaded - the options' CURRENT values say nothing about that
bool rowsUsable(const ft_tracked_batch *tb) { return FT_ROW_FIRST && tb->oCache && tb->hasGrid; }
// The claim iteration of every frame of the batch (see fixedPoint): bursts of passes, one launch per pass for ALL frames, one
// delivery of the flag words + one synchronisation per burst.  A batch has 32 flag positions per burst parity: bursts of up to
// 30 passes (the slowest of many frames needs more passes than one frame does).  With the one-launch resolution
// (c.useResolve; k_resolve_batch: a workgroup per frame walks its points in index order) everything behind the first pass is ONE
// launch; a frame it resolved has all its flag words at -1 and is inert in later passes, and only if it gave up on a frame (a
// candidate list the cache could not hold) do the passes go on - for those frames.
// The iteration is written as two halves around its FIRST host synchronisation: callBegin enqueues everything up to it (the
// whole search when the resolution resolves every frame - the usual case) and returns; callFinish waits, looks at the flag
// words and runs whatever is left.  ft_tracked_batch_submit_* = callBegin, ft_tracked_batch_wait = callFinish.
int callLaunchPass(ft_tracked_batch *tb, FtBatchCall &c, int pass, int fCur, int fPrev, int fReset) {
    ft_context *ctx = tb->ctx;
    hipStream_t st = tb->stream;
    const bool local = c.kind == 2;
    if (local && !c.frustumDone) {  // behind the fill of the claim iteration (which zeroes the counts), in front of the first pass
        c.frustumDone = true;
        tb->evt.begin(ctx->kernelTiming, "kernel.frustum_batch", st);
        const int r = ft_launch_frustum_batch(st, tb->d_arena, c.dJobs, c.n, c.maxM, c.viewingCosLimit, c.logScaleFactor, c.farPoints, c.thFar);
        tb->evt.end(ctx->kernelTiming, st);
        if (r != FT_OK) return r;
    }
    const bool lean = pass > 0 && tb->oCache;
    const bool rows = pass == 0 && rowsUsable(tb);  // (fCur 0, fPrev -1, fReset = half: the kernel's own)
    int r;
    if (local) {
        tb->evt.begin(ctx->kernelTiming, lean ? "kernel.search_local_batch(later pass)" : "kernel.search_local_batch(first pass)", st);
        r = rows   ? ft_launch_search_local_first(st, tb->d_arena, c.dJobs, c.n, c.maxPoints, c.th, c.nnRatio)
            : lean ? ft_launch_search_local_batch_lean(st, tb->d_arena, c.dJobs, c.n, c.maxPoints, pass, fCur, fPrev, fReset, c.th, c.nnRatio)
                   : ft_launch_search_local_batch(st, tb->d_arena, c.dJobs, c.n, c.maxPoints, pass, fCur, fPrev, fReset, c.th, c.nnRatio);
    } else {
        tb->evt.begin(ctx->kernelTiming, lean ? "kernel.search_last_batch(later pass)" : "kernel.search_last_batch(first pass)", st);
        r = rows   ? ft_launch_search_last_first(st, tb->d_arena, c.dJobs, c.n, c.maxPoints, c.th)
            : lean ? ft_launch_search_last_batch_lean(st, tb->d_arena, c.dJobs, c.n, c.maxPoints, pass, fCur, fPrev, fReset, c.th)
                   : ft_launch_search_last_batch(st, tb->d_arena, c.dJobs, c.n, c.maxPoints, pass, fCur, fPrev, fReset, c.th);
    }
    tb->evt.end(ctx->kernelTiming, st);
    if (r == FT_OK && pass == 0 && tb->oCache) {
        tb->evt.begin(ctx->kernelTiming, "kernel.cache_partition_batch", st);
        r = ft_launch_cache_partition_batch(st, tb->d_arena, c.dJobs, c.n, c.maxPoints);
        tb->evt.end(ctx->kernelTiming, st);
    }
    return r;
}

// the flag words, the error words (and the counts) of every frame into pinned host memory; a local-map search's first delivery
// also carries the frustum fields (they do not change from burst to burst).  Records: [n] flags, [n + 1] errors, [n + 2] counts,
// [n + 3 + f] frustum fields of frame f.
int callDeliver(ft_tracked_batch *tb, FtBatchCall &c, int parity, bool first) {
    hipStream_t st = tb->stream;
    if (c.kind == 2 && !c.frustumDone) {  // no frame has keypoints: the frustum fields are still the call's result
        c.frustumDone = true;
        const int r = ft_launch_frustum_batch(st, tb->d_arena, c.dJobs, c.n, c.maxM, c.viewingCosLimit, c.logScaleFactor, c.farPoints, c.thFar);
        if (r != FT_OK) return r;
    }
    const bool frRecs = c.kind == 2 && first && c.haveFrustum && !c.frustumDirect;
    if (c.kind == 2 && first && c.frustumDirect) {
        const int r = ft_launch_gather_batch(st, c.dFrRecs, c.nFrRecs);
        if (r != FT_OK) return r;
    }
    const int nRecs = c.kind == 2 ? (frRecs ? c.n + 3 : 3) : 2;
    return ft_launch_deliver_batch(st, c.dRecs + c.n, nRecs, std::max(frRecs ? c.maxFrWords : 0, FT_BATCH_FLAGS * c.n), parity);
}

int callResolve(ft_tracked_batch *tb, FtBatchCall &c) {
    ft_context *ctx = tb->ctx;
    hipStream_t st = tb->stream;
    const bool local = c.kind == 2;
    tb->evt.begin(ctx->kernelTiming, local ? "kernel.resolve_batch(local map)" : "kernel.resolve_batch(last frame)", st);
    int r = ft_launch_resolve_batch(st, tb->d_arena, c.dJobs, c.n, local ? 1 : 0, c.nnRatio, c.shInts <= 12288 ? c.shInts : 0);
    tb->evt.end(ctx->kernelTiming, st);
    // the writes of the frames it resolved, replayed right behind it (a frame it gave up on waits for the passes)
    tb->evt.begin(ctx->kernelTiming, local ? "kernel.replay_batch(local map)" : "kernel.replay_batch(last frame)", st);
    if (r == FT_OK) r = ft_launch_replay_batch(st, tb->d_arena, c.dJobs, c.n, local ? 1 : 0, 0, c.checkOrientation, c.shInts, /*flagPos=*/0);
    tb->evt.end(ctx->kernelTiming, st);
    return r;
}

constexpr int kFlagHalf = FT_BATCH_FLAGS / 2, kLenMax = kFlagHalf - 2;

// passes [c.nextB, c.len) of burst c.burst, then its delivery
int callRunBurst(ft_tracked_batch *tb, FtBatchCall &c) {
    const int base = kFlagHalf * (c.burst & 1), other = kFlagHalf * ((c.burst + 1) & 1);
    for (int b = c.nextB; b < c.len; b++, c.pass++) {
        const int fPrev = b > 0 ? base + b - 1 : (c.burst > 0 ? other + c.prevLen - 1 : -1);
        int rc = callLaunchPass(tb, c, c.pass, base + b, fPrev, other + b);
        if (rc != FT_OK) return rc;
        c.parity = c.pass & 1;
        if (c.pass == 0 && c.useResolve) {  // the rest of the search in one launch; the host looks at the flag words before it goes on
            rc = callResolve(tb, c);
            if (rc == FT_OK) rc = callDeliver(tb, c, 0, true);
            c.pass++;
            c.nextB = b + 1;
            c.awaitResolve = true;
            return rc;
        }
    }
    c.nextB = c.len;
    // the frames this burst brought to their fixed point are replayed behind it (the kernel looks at the burst's last flag word
    // itself), in front of the delivery: when the host then finds every frame converged the search is complete - no launch and
    // no synchronisation of its own for the replay
    int rc = ft_launch_replay_batch(tb->stream, tb->d_arena, c.dJobs, c.n, c.kind == 2 ? 1 : 0, c.parity, c.checkOrientation, c.shInts,
                                    /*flagPos=*/base + c.len - 1);
    if (rc != FT_OK) return rc;
    return callDeliver(tb, c, c.parity, c.burst == 0 && !c.awaitResolve);
}

int callBegin(ft_tracked_batch *tb, FtBatchCall &c, int burstHint) {
    hipStream_t st = tb->stream;
    const int burstMax = std::min(tb->optPassBurst + 4, kLenMax);
    c.len = burstHint > 0 ? std::min(std::max(burstHint + 1, 4), kLenMax) : burstMax;
    c.pass = c.burst = c.prevLen = c.parity = c.nextB = 0;
    c.simple = c.awaitResolve = c.resolvedAll = false;
    int rc = ft_launch_fill_claims_batch(st, tb->d_arena, c.dJobs, c.n, 27 * c.maxK);
    if (rc != FT_OK) return rc;
    if (c.maxPoints <= 0) {  // nothing to search in any frame: the (empty) results and, for a local-map call, the frustum fields
        c.simple = true;
        rc = ft_launch_replay_batch(st, tb->d_arena, c.dJobs, c.n, c.kind == 2 ? 1 : 0, 0, c.checkOrientation, c.shInts, /*flagPos=*/-1);
        if (rc == FT_OK) rc = callDeliver(tb, c, 0, true);
        c.resolvedAll = true;
        return rc;
    }
    return callRunBurst(tb, c);
}

// the second half: waits for what callBegin enqueued, runs the bursts that are left (none when the resolution resolved every
// frame), has the writes of the frames the passes finished replayed; *passes = claim passes the search took
int callFinish(ft_tracked_batch *tb, FtBatchCall &c, int *passes) {
    ft_context *ctx = tb->ctx;
    hipStream_t st = tb->stream;
    const int *hostFlags = (const int *)(tb->h_out + c.oFlagsOut);
    const int burstMax = std::min(tb->optPassBurst + 4, kLenMax);
    const int maxPasses = 2 * c.maxPoints + 4 + burstMax;
    FT_HIP(hipStreamSynchronize(st));
    *passes = 0;
    if (c.simple) return FT_OK;
    bool firstDelivered = true;  // (callBegin's delivery carried the frustum fields)
    if (c.awaitResolve) {
        bool all = true;
        for (int f = 0; f < c.n && all; f++) all = hostFlags[FT_BATCH_FLAGS * (size_t)f] == -1;
        if (all) {
            c.resolvedAll = true;
            *passes = 2;
            return FT_OK;
        }
        ctx->addStat("tracked_batch.resolve_fallbacks", 1);
        c.awaitResolve = false;
        c.pass = 1;
        int rc = callRunBurst(tb, c);  // the rest of the first burst
        if (rc != FT_OK) return rc;
        FT_HIP(hipStreamSynchronize(st));
    }
    (void)firstDelivered;
    for (;;) {
        const int base = kFlagHalf * (c.burst & 1);
        bool all = true;
        int ranMax = 0;
        for (int f = 0; f < c.n; f++) {
            const int *h = hostFlags + FT_BATCH_FLAGS * (size_t)f + base;
            if (h[c.len - 1] != -1) all = false;
            int ran = 0;
            while (ran < c.len && h[ran] != -1) ran++;
            ranMax = std::max(ranMax, std::min(ran + 1, c.len));
        }
        if (all) {
            c.pass = c.pass - c.len + ranMax;
            break;
        }
        if (c.pass >= maxPasses) {
            ft_set_error("projection search (batch): claim resolution did not converge");
            return FT_ERR_HIP;
        }
        c.prevLen = c.len;
        c.len = std::min(c.len, 6);  // the first burst fell short: short bursts from here (never longer than the one before: the
                                     // flag words beyond a burst's length are not reset by the next one)
        c.burst++;
        c.nextB = 0;
        int rc = callRunBurst(tb, c);
        if (rc != FT_OK) return rc;
        FT_HIP(hipStreamSynchronize(st));
    }
    *passes = c.pass;  // (every frame's writes were replayed behind the burst that brought it to its fixed point: callRunBurst)
    return FT_OK;
}

int checkBatch(const ft_tracked_batch *tb, int n, const char *what) {
    if (!tb) {
        ft_set_error(std::string(what) + ": null batch");
        return FT_ERR_INVALID;
    }
    if (n != tb->nFrames || n <= 0) {
        ft_set_error(std::string(what) + ": n_frames differs from the number of frames uploaded");
        return FT_ERR_INVALID;
    }
    return FT_OK;
}

// LDS ints of k_replay_batch's last-writer table for the uploaded frames (0: a frame beyond the LDS, the table lives in HBM)
int replayShared(const ft_tracked_batch *tb) {
    int maxN = 1;
    for (const FtDevFrame &D : tb->DF) maxN = std::max(maxN, D.N);
    return maxN <= 15360 ? maxN : 0;
}

}  // namespace

extern "C" {

int ft_tracked_batch_create(ft_context *ctx, int max_frames, int max_keypoints, int max_points, ft_tracked_batch **out) {
    FT_REQUIRE(ctx && out && max_frames > 0 && max_keypoints > 0 && max_points > 0, "ft_tracked_batch_create: bad argument");
    FT_REQUIRE(max_frames <= 4096 && max_keypoints < (1 << 24) && max_points < (1 << 22), "ft_tracked_batch_create: capacity out of range");
    int rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    ft_tracked_batch *tb = new ft_tracked_batch();
    tb->ctx = ctx;
    tb->maxFrames = max_frames;
    tb->maxKp = max_keypoints;
    tb->maxPts = max_points;
    const size_t B = (size_t)max_frames;
    Arena a;
    tb->workBytes = (B * batchWorkBytes(max_points) + 4095) & ~(size_t)4095;
    tb->oWork = a.take(tb->workBytes);
    tb->framesBytes = (B * batchFrameBytes(max_keypoints) + 4095) & ~(size_t)4095;
    tb->oFrames = a.take(tb->framesBytes);
    tb->oFlags = a.take(B * FT_BATCH_FLAGS * sizeof(int));
    tb->oCounts = a.take(B * sizeof(int));
    tb->oReplayed = a.take(B * sizeof(int));
    tb->oErr = a.take(B * sizeof(int));
    tb->gridStride = (gridBytes(max_keypoints) + 255) & ~(size_t)255;
    tb->oGrid = a.take(B * tb->gridStride);
    tb->claimStride = (batchClaimBytes(max_keypoints, max_points) + 255) & ~(size_t)255;
    tb->oClaims = a.take(B * tb->claimStride);
    if (searchCacheOn(ctx)) {
        tb->cacheStride = searchCacheBytes(max_points);
        tb->oCache = a.take(B * tb->cacheStride);
    }
    tb->arenaBytes = a.off;
    // results of a search (per point) or of bind_fisheye (per keypoint: match tables, mvDepth, mvStereo3Dpoints)
    // (+ a search's assignments: 4 bytes per keypoint, and its match count)
    tb->outBytes = B * (std::max(batchOutBytes(max_points), 20 * (size_t)max_keypoints + 8 * 64) + 4 * (size_t)max_keypoints + 128) +
                   B * FT_BATCH_FLAGS * sizeof(int) + 4096;
    hipError_t e = hipMalloc((void **)&tb->d_arena, tb->arenaBytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&tb->h_in, tb->workBytes + tb->framesBytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&tb->h_out, tb->outBytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&tb->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&tb->evGather, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&tb->evMirror, hipEventDisableTiming);
    if (e != hipSuccess) {
        ft_tracked_batch_destroy(tb);
        return ft_hip_fail(e, "ft_tracked_batch_create", __FILE__, __LINE__);
    }
    tb->counted = true;
    ctx->liveObjects++;
    *out = tb;
    return FT_OK;
}

int ft_tracked_batch_destroy(ft_tracked_batch *tb) {
    if (!tb) return FT_OK;
    ft_set_device(tb->ctx);
    if (tb->stream) {
        hipStreamSynchronize(tb->stream);
        hipStreamDestroy(tb->stream);
    }
    if (tb->evMirror) hipEventDestroy(tb->evMirror);
    if (tb->evGather) {  // an extractor bound to this batch may still hold the event for its next batch: it goes with the context
        std::lock_guard<std::mutex> lk(tb->ctx->hostAllocMutex);
        tb->ctx->retiredEvents.push_back(tb->evGather);
    }
    if (tb->d_arena) hipFree(tb->d_arena);
    if (tb->h_in) hipHostFree(tb->h_in);
    if (tb->h_out) hipHostFree(tb->h_out);
    tb->evt.destroy();
    if (tb->counted) tb->ctx->liveObjects--;
    delete tb;
    return FT_OK;
}

int ft_tracked_batch_upload(ft_tracked_batch *tb, int n_frames, const ft_frame_view *frames) {
    FT_REQUIRE(tb && frames && n_frames > 0 && n_frames <= tb->maxFrames, "ft_tracked_batch_upload: bad argument");
    int nlevelsMax = 1;
    bool twoCam = false;
    for (int f = 0; f < n_frames; f++) {
        int rc = checkFrame(&frames[f]);
        if (rc != FT_OK) return rc;
        FT_REQUIRE(frames[f].N <= tb->maxKp, "ft_tracked_batch_upload: more keypoints than the batch was created for");
        nlevelsMax = std::max(nlevelsMax, frames[f].nlevels);
        twoCam = twoCam || frames[f].Nleft != -1;
    }
    ft_context *ctx = tb->ctx;
    int rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(tb->mu);
    FT_REQUIRE(tb->call.kind == 0, "ft_tracked_batch_upload: a submitted search of this batch has not been waited for (ft_tracked_batch_wait)");
    FtTimer tAll;
    hipStream_t st = tb->stream;
    bool wantGrid;
    {
        std::lock_guard<std::mutex> lo(ctx->matchMutex);
        wantGrid = ctx->tuning.search_grid != 0;
    }
    tb->hasGrid = false;  // (until the launch that builds the grids of THESE frames is enqueued)
    FT_HIP(hipStreamSynchronize(st));  // the pinned mirror is repacked: nothing of an earlier call may still read it
    // layout of the frames region: the holder_obs arrays of all frames first (contiguous: refreshed after every search by one
    // copy), then every frame's arrays
    Arena a;
    tb->holderOff.assign(n_frames, 0);
    tb->holderBegin = a.off;
    for (int f = 0; f < n_frames; f++) tb->holderOff[f] = a.take(sizeof(int) * std::max(frames[f].N, 1));
    tb->holderEnd = a.off;
    struct Lay {
        size_t keys, keysR, desc, uright, l2r, r2l;
    };
    std::vector<Lay> lay(n_frames);
    for (int f = 0; f < n_frames; f++) {
        const ft_frame_view &F = frames[f];
        const int nL = F.Nleft == -1 ? F.N : F.Nleft, nR = F.Nleft == -1 ? 0 : F.N - F.Nleft;
        lay[f].keys = a.take(sizeof(ft_keypoint) * std::max(nL, 1));
        lay[f].keysR = a.take(sizeof(ft_keypoint) * std::max(nR, 1));
        lay[f].desc = a.take((size_t)32 * std::max(F.N, 1));
        lay[f].uright = a.take(sizeof(float) * std::max(F.N, 1));
        lay[f].l2r = a.take(sizeof(int) * std::max(nL, 1));
        lay[f].r2l = a.take(sizeof(int) * std::max(nR, 1));
    }
    FT_REQUIRE(a.off <= tb->framesBytes, "ft_tracked_batch_upload: frames region too small");
    tb->nFrames = n_frames;
    tb->DF.assign(n_frames, FtDevFrame());
    uint8_t *pinF = tb->h_in + tb->workBytes, *devF = tb->d_arena + tb->oFrames;
    FtBatchJob *hJobs = (FtBatchJob *)tb->h_in;
    FT_REQUIRE((size_t)n_frames * sizeof(FtBatchJob) <= tb->workBytes, "ft_tracked_batch_upload: work region too small");
    // the caller's arrays are pageable as a rule: packed into the pinned mirror by the context's host threads, one frame each
    const std::function<void(int, int)> stage = [&](int f, int) {
        const ft_frame_view &F = frames[f];
        const int nL = F.Nleft == -1 ? F.N : F.Nleft, nR = F.Nleft == -1 ? 0 : F.N - F.Nleft;
        if (nL) memcpy(pinF + lay[f].keys, F.keys, sizeof(ft_keypoint) * nL);
        if (nR) memcpy(pinF + lay[f].keysR, F.keys_right, sizeof(ft_keypoint) * nR);
        if (F.N) memcpy(pinF + lay[f].desc, F.descriptors, (size_t)32 * F.N);
        if (F.uright && F.N) memcpy(pinF + lay[f].uright, F.uright, sizeof(float) * F.N);
        if (F.Nleft != -1) {
            if (nL) memcpy(pinF + lay[f].l2r, F.left_to_right, sizeof(int) * nL);
            if (nR) memcpy(pinF + lay[f].r2l, F.right_to_left, sizeof(int) * nR);
        }
        if (F.N) memcpy(pinF + tb->holderOff[f], F.holder_obs, sizeof(int) * F.N);
        FtDevFrame &D = tb->DF[f];
        D = devFrameConstants(&F);
        D.keys = (const ft_keypoint *)(devF + lay[f].keys);
        D.keysR = (const ft_keypoint *)(devF + lay[f].keysR);
        D.desc = devF + lay[f].desc;
        D.uright = F.uright ? (const float *)(devF + lay[f].uright) : nullptr;
        D.holderObs = (const int *)(devF + tb->holderOff[f]);
        D.l2r = F.Nleft != -1 ? (const int *)(devF + lay[f].l2r) : nullptr;
        D.r2l = F.Nleft != -1 ? (const int *)(devF + lay[f].r2l) : nullptr;
        if (wantGrid) pointGrid(D, (int *)(tb->d_arena + tb->oGrid + (size_t)f * tb->gridStride));  // (k_build_grid_batch fills it)
        memset(&hJobs[f], 0, sizeof(FtBatchJob));
        hJobs[f].F = D;
    };
    ctx->pool->parallel_for(n_frames, stage);
    FT_HIP(hipMemcpyAsync(tb->d_arena + tb->oWork, tb->h_in, (size_t)n_frames * sizeof(FtBatchJob), hipMemcpyHostToDevice, st));
    FT_HIP(hipMemcpyAsync(devF, pinF, a.off, hipMemcpyHostToDevice, st));
    FT_HIP(hipEventRecord(tb->evMirror, st));
    if (wantGrid) {
        rc = ft_launch_build_grid_batch(st, tb->d_arena, (const FtBatchJob *)(tb->d_arena + tb->oWork), n_frames, nlevelsMax, twoCam);
        if (rc != FT_OK) return rc;
        tb->hasGrid = true;
    }
    ctx->addStat("tracked_batch.upload.total", tAll.ms());
    return FT_OK;
}

int ft_tracked_batch_holder_obs(ft_tracked_batch *tb, int frame, int *holder_obs) {
    FT_REQUIRE(tb && holder_obs, "ft_tracked_batch_holder_obs: bad argument");
    std::lock_guard<std::mutex> lk(tb->mu);  // (upload / bind_fisheye reassign the vectors)
    FT_REQUIRE(frame >= 0 && frame < tb->nFrames, "ft_tracked_batch_holder_obs: bad argument");
    FT_REQUIRE(tb->call.kind == 0, "ft_tracked_batch_holder_obs: a submitted search of this batch has not been waited for (ft_tracked_batch_wait)");
    int rc = ft_set_device(tb->ctx);
    if (rc != FT_OK) return rc;
    const int N = tb->DF[frame].N;
    if (N > 0) {  // (the array lives in HBM; the copy is ordered behind the batch's searches on its stream)
        FT_HIP(hipMemcpyAsync(holder_obs, tb->d_arena + tb->oFrames + tb->holderOff[frame], sizeof(int) * (size_t)N, hipMemcpyDeviceToHost, tb->stream));
        FT_HIP(hipStreamSynchronize(tb->stream));
    }
    return FT_OK;
}

}  // extern "C"

namespace {

// May the device read [p, p + bytes) in place?  A block of ft_host_malloc is known without asking the runtime; anything else is
// asked about (hipHostMalloc / hipHostRegister memory of the application qualifies, at a few microseconds per array).
bool readableInPlace(ft_context *ctx, const void *p, size_t bytes) {
    if (!p || bytes == 0) return true;
    return ft_host_block_contains(ctx, p, bytes) || ft_is_pinned_host_range(p, bytes);
}

// the records of a call's head in the pinned mirror: jobs | delivery records | gather records (the gather records only when the
// caller's arrays are read in place)
struct CallHead {
    size_t oJobs, oRecs, oGather;
    FtBatchJob *hJobs;
    FtDeliverRec *hRecs;
    FtGatherRec *hGather;
};
CallHead layoutHead(ft_tracked_batch *tb, Arena &a, int n, int nRecs, int nGather) {
    CallHead H;
    H.oJobs = a.take((size_t)n * sizeof(FtBatchJob));
    H.oRecs = a.take((size_t)nRecs * sizeof(FtDeliverRec));
    H.oGather = a.take((size_t)std::max(nGather, 1) * sizeof(FtGatherRec));
    H.hJobs = (FtBatchJob *)(tb->h_in + H.oJobs);
    H.hRecs = (FtDeliverRec *)(tb->h_in + H.oRecs);
    H.hGather = (FtGatherRec *)(tb->h_in + H.oGather);
    return H;
}

int requireIdle(ft_tracked_batch *tb, const char *what) {
    if (tb->call.kind != 0) {
        ft_set_error(std::string(what) + ": a submitted search of this batch has not been waited for (ft_tracked_batch_wait)");
        return FT_ERR_INVALID;
    }
    return FT_OK;
}

// SearchByProjection(CurrentFrame, LastFrame) of every frame, first half.  The point arrays are read IN PLACE by the device when
// every one of them lies in pinned host memory (one gather launch, no host copy; they must then stay unchanged until the wait
// returns); otherwise the host threads of the context pack them into the batch's pinned mirror and one copy takes them up.
int submitLastFrame(ft_tracked_batch *tb, int n, const ft_last_points *L, const FtPose *poses, const FtPose *trls, bool needTrl, float th,
                    const int *forward, const int *backward, int check_orientation, int *const *assign, int *n_matches) {
    int rc = requireIdle(tb, "ft_tracked_batch_search_last_frame");
    if (rc != FT_OK) return rc;
    rc = checkBatch(tb, n, "ft_tracked_batch_search_last_frame");
    if (rc != FT_OK) return rc;
    FT_REQUIRE(L && assign, "ft_tracked_batch_search_last_frame: null argument");
    ft_context *ctx = tb->ctx;
    snapshotTuning(tb);
    bool inPlace = true;
    for (int f = 0; f < n; f++) {
        FT_REQUIRE(!needTrl || trls || tb->DF[f].Nleft == -1, "ft_tracked_batch_search_last_frame_se3: a two-camera frame needs Trl");
        FT_REQUIRE(assign[f], "ft_tracked_batch_search_last_frame: null assign array");
        rc = checkLastPoints(&L[f], 0, tb->maxPts, "batch");
        if (rc != FT_OK) return rc;
        const size_t m = (size_t)L[f].N;
        inPlace = inPlace && readableInPlace(ctx, L[f].valid, m) && readableInPlace(ctx, L[f].world_pos, 12 * m) &&
                  readableInPlace(ctx, L[f].descriptors, 32 * m) && readableInPlace(ctx, L[f].observations, 4 * m) &&
                  readableInPlace(ctx, L[f].octave, 4 * m) && readableInPlace(ctx, L[f].angle, 4 * m);
    }
    if (!inPlace)  // the host reads the arrays anyway: octaves checked here (in place: k_last_project_batch checks them, the wait reports)
        for (int f = 0; f < n; f++)
            if ((rc = checkLastPoints(&L[f], tb->DF[f].nlevels, tb->maxPts, "batch")) != FT_OK) return rc;
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    FtBatchCall &c = tb->call;
    c = FtBatchCall();
    c.assignDirect = true;
    for (int f = 0; f < n; f++) c.assignDirect = c.assignDirect && readableInPlace(ctx, assign[f], 4 * (size_t)std::max(tb->DF[f].N, 1));
    hipStream_t st = tb->stream;
    // layout of the call in the work region: job records | delivery records | gather records | per frame the point arrays
    Arena a;
    const CallHead H = layoutHead(tb, a, n, n + 2, inPlace ? 6 * n : 0);
    const size_t headEnd = a.off;
    struct Lay : LastLayout {
        size_t ang, proj;
    };
    std::vector<Lay> lay(n);
    Arena o;  // results in tb->h_out: flag words, error words, match counts, every frame's assignments (k_replay_batch writes them there)
    c.oFlagsOut = o.take((size_t)n * FT_BATCH_FLAGS * sizeof(int));
    c.oErrOut = o.take((size_t)n * sizeof(int));
    c.oNmOut = o.take((size_t)n * sizeof(int));
    c.outAssign.resize(n);
    for (int f = 0; f < n; f++) {
        const size_t M = (size_t)std::max(L[f].N, 1);
        (LastLayout &)lay[f] = layoutLast(a, M);
        lay[f].ang = a.take(4 * M);
        c.outAssign[f] = o.take(4 * (size_t)std::max(tb->DF[f].N, 1));
    }
    const size_t inputEnd = a.off;  // what follows is device-only: the projections
    for (int f = 0; f < n; f++) lay[f].proj = a.take(sizeof(FtLastProj) * (size_t)std::max(L[f].N, 1));
    FT_REQUIRE(a.off <= tb->workBytes && o.off <= tb->outBytes, "tracked batch work arena too small");
    uint8_t *pin = tb->h_in, *dev = tb->d_arena + tb->oWork;
    FT_HIP(hipEventSynchronize(tb->evMirror));  // (the pinned mirror: the previous call's copy out of it - not the whole stream, whose
                                                // kernels - a bind_fisheye enqueued just before - may run on while this call is staged)
    const std::function<void(int, int)> stage = [&](int f, int) {
        const ft_last_points &P = L[f];
        const size_t M = (size_t)P.N;
        const int N = tb->DF[f].N;
        if (inPlace) {
            FtGatherRec *G = H.hGather + 6 * (size_t)f;
            G[0] = {dev + lay[f].valid, P.valid, (unsigned)M};
            G[1] = {dev + lay[f].pos, P.world_pos, (unsigned)(12 * M)};
            G[2] = {dev + lay[f].desc, P.descriptors, (unsigned)(32 * M)};
            G[3] = {dev + lay[f].obs, P.observations, (unsigned)(4 * M)};
            G[4] = {dev + lay[f].oct, P.octave, (unsigned)(4 * M)};
            G[5] = {dev + lay[f].ang, P.angle, (unsigned)(4 * M)};
        } else if (M) {
            stageLast(&P, lay[f], pin);
            memcpy(pin + lay[f].ang, P.angle, 4 * M);
        }
        FtBatchJob &J = H.hJobs[f];
        memset(&J, 0, sizeof J);
        J.F = tb->DF[f];
        if (trls) setTrl(J.F, trls[f]);
        batchClaims(tb, f, N, N > 0 ? (int)M : 0, J);
        J.obs = (const int *)(dev + lay[f].obs);
        J.L = devLast((int)M, lay[f], dev);
        J.L.angle = (const float *)(dev + lay[f].ang);
        J.proj = (FtLastProj *)(dev + lay[f].proj);
        J.Tcw = poses[f];
        J.forward = forward ? forward[f] : 0;
        J.backward = backward ? backward[f] : 0;
        J.assignOut = c.assignDirect ? assign[f] : (int *)(tb->h_out + c.outAssign[f]);
        J.nmOut = (int *)(tb->h_out + c.oNmOut) + f;
        memset(&H.hRecs[f], 0, sizeof(FtDeliverRec));  // (the points' results stay on the device: k_replay_batch turns them into assignments there)
    };
    if (inPlace)
        for (int f = 0; f < n; f++) stage(f, 0);  // (a few hundred bytes per frame: not worth waking the pool)
    else
        ctx->pool->parallel_for(n, stage);
    for (int f = 0; f < n; f++) {
        c.maxPoints = std::max(c.maxPoints, H.hJobs[f].nPoints);
        if (H.hJobs[f].nPoints > 0) c.maxK = std::max(c.maxK, H.hJobs[f].K);
    }
    H.hRecs[n] = {tb->h_out + c.oFlagsOut, {tb->d_arena + tb->oFlags, tb->d_arena + tb->oFlags}, FT_BATCH_FLAGS * n};
    H.hRecs[n + 1] = {tb->h_out + c.oErrOut, {tb->d_arena + tb->oErr, tb->d_arena + tb->oErr}, n};
    ctx->addStat("tracked_batch.search_last_frame.stage", c.tAll.ms());
    FT_HIP(hipMemcpyAsync(dev, pin, inPlace ? headEnd : inputEnd, hipMemcpyHostToDevice, st));
    FT_HIP(hipEventRecord(tb->evMirror, st));
    if (inPlace) {
        rc = ft_launch_gather_batch(st, (const FtGatherRec *)(dev + H.oGather), 6 * n);
        if (rc != FT_OK) return rc;
    }
    c.n = n;
    c.dJobs = (const FtBatchJob *)(dev + H.oJobs);
    c.dRecs = (const FtDeliverRec *)(dev + H.oRecs);
    c.th = th;
    c.checkOrientation = check_orientation;
    c.useResolve = rowsUsable(tb) && resolveWanted(tb, n);
    c.shInts = replayShared(tb);
    c.assign.assign(assign, assign + n);
    c.nMatches = n_matches;
    c.kind = 1;
    rc = callBegin(tb, c, tb->passesLast);
    if (rc != FT_OK) c.kind = 0;
    return rc;
}

// isInFrustum + SearchByProjection(Frame, local map points) of every frame, first half (inputs as submitLastFrame)
int submitLocalMap(ft_tracked_batch *tb, int n, const ft_frame_pose *poses, const ft_map_points *P, float viewing_cos_limit,
                   float log_scale_factor, float th, float nn_ratio, int far_points, float th_far_points,
                   const ft_frustum_result *frustum, int *n_to_match, int *const *assign, int *n_matches) {
    int rc = requireIdle(tb, "ft_tracked_batch_track_local_map");
    if (rc != FT_OK) return rc;
    rc = checkBatch(tb, n, "ft_tracked_batch_track_local_map");
    if (rc != FT_OK) return rc;
    snapshotTuning(tb);
    FT_REQUIRE(poses && P && assign, "ft_tracked_batch_track_local_map: null argument");
    ft_context *ctx = tb->ctx;
    bool inPlace = true;
    for (int f = 0; f < n; f++) {
        rc = checkMapPoints(&P[f], true);
        if (rc != FT_OK) return rc;
        FT_REQUIRE(P[f].M <= tb->maxPts, "map point count beyond the batch's capacity");
        FT_REQUIRE(assign[f], "ft_tracked_batch_track_local_map: null assign array");
        const size_t m = (size_t)P[f].M;
        inPlace = inPlace && readableInPlace(ctx, P[f].skip, m) && readableInPlace(ctx, P[f].world_pos, 12 * m) &&
                  readableInPlace(ctx, P[f].normal, 12 * m) && readableInPlace(ctx, P[f].max_distance, 4 * m) &&
                  readableInPlace(ctx, P[f].min_distance, 4 * m) && readableInPlace(ctx, P[f].descriptors, 32 * m) &&
                  readableInPlace(ctx, P[f].observations, 4 * m);
    }
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    FtBatchCall &c = tb->call;
    c = FtBatchCall();
    c.assignDirect = true;
    for (int f = 0; f < n; f++) c.assignDirect = c.assignDirect && readableInPlace(ctx, assign[f], 4 * (size_t)std::max(tb->DF[f].N, 1));
    hipStream_t st = tb->stream;
    Arena a;
    // the frustum fields: straight into the caller's arrays when every one of them lies in pinned memory (a scatter launch, 12
    // records per frame, behind k_frustum_batch), else through the batch's result buffer and the host's copies (unpackFrustum)
    bool frDirect = frustum != nullptr;
    auto field_ptrs = [](const ft_frustum_result &R, void *out[12]) {
        void *p[12] = {R.in_view, R.in_view_r, R.level, R.level_r, R.view_cos, R.view_cos_r, R.proj_x, R.proj_y, R.proj_xr, R.proj_yr, R.depth, R.depth_r};
        for (int k = 0; k < 12; k++) out[k] = p[k];
    };
    static const int kFieldBytes[12] = {1, 1, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4};
    for (int f = 0; f < n && frDirect; f++) {
        void *fp[12];
        field_ptrs(frustum[f], fp);
        for (int k = 0; k < 12; k++) frDirect = frDirect && readableInPlace(ctx, fp[k], (size_t)kFieldBytes[k] * (size_t)P[f].M);
    }
    const CallHead H = layoutHead(tb, a, n, 2 * n + 3, (inPlace ? 7 * n : 0) + (frDirect ? 12 * n : 0));
    const size_t headEnd = a.off;
    struct Lay {
        size_t fIn0, fOutEnd, desc, obs;
    };
    std::vector<Lay> lay(n);
    c.FL.resize(n);
    c.fInEnd.resize(n);
    c.outAssign.resize(n);
    c.outFr.resize(n);
    c.M.resize(n);
    Arena o;
    c.oFlagsOut = o.take((size_t)n * FT_BATCH_FLAGS * sizeof(int));
    c.oErrOut = o.take((size_t)n * sizeof(int));
    c.oCountsOut = o.take((size_t)n * sizeof(int));
    c.oNmOut = o.take((size_t)n * sizeof(int));
    // inputs of all frames first (one H2D copy when they are staged), then the frustum outputs (device only)
    for (int f = 0; f < n; f++) {
        const size_t M = (size_t)std::max(P[f].M, 1);
        lay[f].desc = a.take(32 * M);
        lay[f].obs = a.take(4 * M);
        c.M[f] = P[f].M;
    }
    // (FrustumLayout interleaves a frame's inputs and outputs: a staged copy covers both, the outputs' share is ~40 %)
    for (int f = 0; f < n; f++) {
        lay[f].fIn0 = a.off;
        layoutFrustum(P[f].M, P[f].skip != nullptr, a, c.FL[f], &c.fInEnd[f]);
        lay[f].fOutEnd = a.off;
        c.outAssign[f] = o.take(4 * (size_t)std::max(tb->DF[f].N, 1));
        c.outFr[f] = o.take(lay[f].fOutEnd - c.fInEnd[f]);
    }
    FT_REQUIRE(a.off <= tb->workBytes && o.off <= tb->outBytes, "tracked batch work arena too small");
    uint8_t *pin = tb->h_in, *dev = tb->d_arena + tb->oWork;
    FT_HIP(hipEventSynchronize(tb->evMirror));
    const std::function<void(int, int)> stage = [&](int f, int) {
        const ft_map_points &Q = P[f];
        const size_t M = (size_t)Q.M;
        const int N = tb->DF[f].N;
        const FrustumLayout &FL = c.FL[f];
        if (inPlace) {
            FtGatherRec *G = H.hGather + 7 * (size_t)f;
            G[0] = {dev + FL.skip, Q.skip, (unsigned)(Q.skip ? M : 0)};
            G[1] = {dev + FL.pos, Q.world_pos, (unsigned)(12 * M)};
            G[2] = {dev + FL.nrm, Q.normal, (unsigned)(12 * M)};
            G[3] = {dev + FL.maxd, Q.max_distance, (unsigned)(4 * M)};
            G[4] = {dev + FL.mind, Q.min_distance, (unsigned)(4 * M)};
            G[5] = {dev + lay[f].desc, Q.descriptors, (unsigned)(32 * M)};
            G[6] = {dev + lay[f].obs, Q.observations, (unsigned)(4 * M)};
        } else {
            stageFrustum(&Q, FL, pin);
            if (M) {
                memcpy(pin + lay[f].desc, Q.descriptors, 32 * M);
                memcpy(pin + lay[f].obs, Q.observations, 4 * M);
            }
        }
        FtBatchJob &J = H.hJobs[f];
        memset(&J, 0, sizeof J);
        J.F = tb->DF[f];
        batchClaims(tb, f, N, N > 0 ? (int)M : 0, J);
        J.obs = (const int *)(dev + lay[f].obs);
        J.MP = devMapPoints(&Q, FL, dev);
        J.T = frustumPose_fromDev(J.F, &poses[f]);
        J.O = devFrustumOut(FL, dev);
        J.O.count = (int *)(tb->d_arena + tb->oCounts) + f;
        J.P = localPointsOf(J.O, (int)M, dev + lay[f].desc);
        J.assignOut = c.assignDirect ? assign[f] : (int *)(tb->h_out + c.outAssign[f]);
        J.nmOut = (int *)(tb->h_out + c.oNmOut) + f;
        if (frDirect) {
            FtGatherRec *G = H.hGather + (inPlace ? 7 * (size_t)n : 0) + 12 * (size_t)f;
            void *fp[12];
            field_ptrs(frustum[f], fp);
            const size_t srcOff[12] = {FL.inV, FL.inVR, FL.lvl, FL.lvlR, FL.vc, FL.vcR, FL.px, FL.py, FL.pxr, FL.pyr, FL.dep, FL.depR};
            for (int k = 0; k < 12; k++) G[k] = {fp[k], dev + srcOff[k], (unsigned)(fp[k] ? (size_t)kFieldBytes[k] * M : 0)};
        }
        memset(&H.hRecs[f], 0, sizeof(FtDeliverRec));
        FtDeliverRec &R2 = H.hRecs[n + 3 + f];  // (the frustum fields do not change from burst to burst: delivered with the first one)
        R2.dst = tb->h_out + c.outFr[f];
        R2.src[0] = R2.src[1] = dev + c.fInEnd[f];
        R2.words = M ? (int)((lay[f].fOutEnd - c.fInEnd[f]) / 4) : 0;
    };
    if (inPlace)
        for (int f = 0; f < n; f++) stage(f, 0);
    else
        ctx->pool->parallel_for(n, stage);
    for (int f = 0; f < n; f++) {
        c.maxPoints = std::max(c.maxPoints, H.hJobs[f].nPoints);
        c.maxM = std::max(c.maxM, P[f].M);
        if (H.hJobs[f].nPoints > 0) c.maxK = std::max(c.maxK, H.hJobs[f].K);
        c.maxFrWords = std::max(c.maxFrWords, H.hRecs[n + 3 + f].words);
    }
    H.hRecs[n] = {tb->h_out + c.oFlagsOut, {tb->d_arena + tb->oFlags, tb->d_arena + tb->oFlags}, FT_BATCH_FLAGS * n};
    H.hRecs[n + 1] = {tb->h_out + c.oErrOut, {tb->d_arena + tb->oErr, tb->d_arena + tb->oErr}, n};
    H.hRecs[n + 2] = {tb->h_out + c.oCountsOut, {tb->d_arena + tb->oCounts, tb->d_arena + tb->oCounts}, n};
    ctx->addStat("tracked_batch.track_local_map.stage", c.tAll.ms());
    FT_HIP(hipMemcpyAsync(dev, pin, inPlace ? headEnd : a.off, hipMemcpyHostToDevice, st));
    FT_HIP(hipEventRecord(tb->evMirror, st));
    if (inPlace) {
        rc = ft_launch_gather_batch(st, (const FtGatherRec *)(dev + H.oGather), 7 * n);
        if (rc != FT_OK) return rc;
    }
    c.n = n;
    c.dJobs = (const FtBatchJob *)(dev + H.oJobs);
    c.dRecs = (const FtDeliverRec *)(dev + H.oRecs);
    c.th = th;
    c.nnRatio = nn_ratio;
    c.viewingCosLimit = viewing_cos_limit;
    c.logScaleFactor = log_scale_factor;
    c.farPoints = far_points;
    c.thFar = th_far_points;
    c.useResolve = rowsUsable(tb) && resolveWanted(tb, n);
    c.shInts = replayShared(tb);
    c.assign.assign(assign, assign + n);
    c.nMatches = n_matches;
    c.nToMatch = n_to_match;
    c.haveFrustum = frustum != nullptr;
    c.frustumDirect = frDirect;
    c.dFrRecs = (const FtGatherRec *)(dev + H.oGather) + (inPlace ? 7 * (size_t)n : 0);
    c.nFrRecs = frDirect ? 12 * n : 0;
    if (frustum) c.frustum.assign(frustum, frustum + n);
    c.kind = 2;
    rc = callBegin(tb, c, tb->passesLocal);
    if (rc != FT_OK) c.kind = 0;
    return rc;
}

// the second half of either search: waits for the device, runs the claim passes the resolution left (none as a rule), hands the
// results to the caller's arrays
int waitCall(ft_tracked_batch *tb) {
    FtBatchCall &c = tb->call;
    if (c.kind == 0) return FT_OK;
    ft_context *ctx = tb->ctx;
    int rc = ft_set_device(ctx);
    const int kind = c.kind, n = c.n;
    const char *name = kind == 1 ? "search_last_frame" : "track_local_map";
    if (rc != FT_OK) {
        c.kind = 0;
        return rc;
    }
    FtTimer tDev;
    int passes = 0;
    rc = callFinish(tb, c, &passes);
    c.kind = 0;  // (whatever happened, the batch is free for the next call)
    if (rc != FT_OK) return rc;
    ctx->addStat((std::string("tracked_batch.") + name + ".device").c_str(), tDev.ms());
    tb->evt.resolve(ctx);
    (kind == 1 ? tb->passesLast : tb->passesLocal) = passes;
    FtTimer tRep;
    const int *hErr = (const int *)(tb->h_out + c.oErrOut);
    for (int f = 0; f < n; f++)
        if (hErr[f] & FT_JOB_ERR_OCTAVE) {
            ft_set_error("last-frame octave out of range");
            return FT_ERR_INVALID;
        }
    // what is left for the host: the assignments (and frustum fields) out of the pinned result buffer into the caller's arrays
    const int *hNm = (const int *)(tb->h_out + c.oNmOut), *hCounts = (const int *)(tb->h_out + c.oCountsOut);
    const std::function<void(int, int)> finish = [&](int f, int) {
        const int N = tb->DF[f].N;
        if (N > 0 && !c.assignDirect) memcpy(c.assign[f], tb->h_out + c.outAssign[f], sizeof(int) * (size_t)N);
        if (c.nMatches) c.nMatches[f] = hNm[f];
        if (kind == 2) {
            const int M = c.M[f];
            // unpackFrustum reads the count through the layout; the batch keeps the counts of all frames in one block
            if (M > 0 && c.haveFrustum && !c.frustumDirect) unpackFrustum(M, c.FL[f], c.fInEnd[f], tb->h_out + c.outFr[f], &c.frustum[f], nullptr);
            if (c.nToMatch) c.nToMatch[f] = M > 0 ? hCounts[f] : 0;
        }
    };
    if (n <= 8) for (int f = 0; f < n; f++) finish(f, 0);
    else ctx->pool->parallel_for(n, finish);
    ctx->addStat((std::string("tracked_batch.") + name + ".replay").c_str(), tRep.ms());
    ctx->addStat((std::string("tracked_batch.") + name + ".total").c_str(), c.tAll.ms());
    ctx->addStat((std::string("tracked_batch.") + name + ".passes").c_str(), passes);
    ctx->addStat((std::string("tracked_batch.") + name + ".frames").c_str(), n);
    return FT_OK;
}

// the three searches' entry points in both forms: submit alone (ft_tracked_batch_submit_*), or submit + wait
int searchLastMatrices(ft_tracked_batch *tb, int n_frames, const ft_last_points *L, const float *Tcw, float th, const int *forward,
                       const int *backward, int check_orientation, int *const *assign, int *n_matches, bool wait) {
    FT_REQUIRE(tb && Tcw && n_frames > 0, "ft_tracked_batch_search_last_frame: null batch or pose");
    std::vector<FtPose> poses(n_frames);
    for (int f = 0; f < n_frames; f++) poses[f] = poseOfMatrix(Tcw + 12 * (size_t)f);
    std::lock_guard<std::mutex> lk(tb->mu);  // (before anything of the batch is read: upload / bind_fisheye reassign it)
    const int rc = submitLastFrame(tb, n_frames, L, poses.data(), nullptr, false, th, forward, backward, check_orientation, assign, n_matches);
    return rc == FT_OK && wait ? waitCall(tb) : rc;
}
int searchLastSe3(ft_tracked_batch *tb, int n_frames, const ft_last_points *L, const ft_se3 *Tcw, const ft_se3 *Trl, float th,
                  const int *forward, const int *backward, int check_orientation, int *const *assign, int *n_matches, bool wait) {
    FT_REQUIRE(tb && Tcw && n_frames > 0, "ft_tracked_batch_search_last_frame_se3: bad argument");
    std::vector<FtPose> poses(n_frames), trls(n_frames);
    for (int f = 0; f < n_frames; f++) {  // (the batch's own state - frame count, camera counts - is checked under its lock: submitLastFrame)
        const FtPose *unused;
        const int rc = posesFromSe3(&Tcw[f], Trl ? &Trl[f] : nullptr, false, "", poses[f], trls[f], &unused);
        if (rc != FT_OK) return rc;
    }
    std::lock_guard<std::mutex> lk(tb->mu);
    const int rc = submitLastFrame(tb, n_frames, L, poses.data(), Trl ? trls.data() : nullptr, true, th, forward, backward, check_orientation,
                                   assign, n_matches);
    return rc == FT_OK && wait ? waitCall(tb) : rc;
}
int trackLocalMap(ft_tracked_batch *tb, int n_frames, const ft_frame_pose *poses, const ft_map_points *P, float viewing_cos_limit,
                  float log_scale_factor, float th, float nn_ratio, int far_points, float th_far_points, const ft_frustum_result *frustum,
                  int *n_to_match, int *const *assign, int *n_matches, bool wait) {
    FT_REQUIRE(tb, "ft_tracked_batch_track_local_map: null batch");
    std::lock_guard<std::mutex> lk(tb->mu);
    const int rc = submitLocalMap(tb, n_frames, poses, P, viewing_cos_limit, log_scale_factor, th, nn_ratio, far_points, th_far_points, frustum,
                                  n_to_match, assign, n_matches);
    return rc == FT_OK && wait ? waitCall(tb) : rc;
}
}  // namespace

extern "C" {

int ft_tracked_batch_submit_search_last_frame(ft_tracked_batch *tb, int n_frames, const ft_last_points *L, const float *Tcw, float th,
                                              const int *forward, const int *backward, int check_orientation, int *const *assign,
                                              int *n_matches) {
    return searchLastMatrices(tb, n_frames, L, Tcw, th, forward, backward, check_orientation, assign, n_matches, false);
}

int ft_tracked_batch_submit_search_last_frame_se3(ft_tracked_batch *tb, int n_frames, const ft_last_points *L, const ft_se3 *Tcw,
                                                  const ft_se3 *Trl, float th, const int *forward, const int *backward,
                                                  int check_orientation, int *const *assign, int *n_matches) {
    return searchLastSe3(tb, n_frames, L, Tcw, Trl, th, forward, backward, check_orientation, assign, n_matches, false);
}

int ft_tracked_batch_submit_track_local_map(ft_tracked_batch *tb, int n_frames, const ft_frame_pose *poses, const ft_map_points *P,
                                            float viewing_cos_limit, float log_scale_factor, float th, float nn_ratio, int far_points,
                                            float th_far_points, const ft_frustum_result *frustum, int *n_to_match, int *const *assign,
                                            int *n_matches) {
    return trackLocalMap(tb, n_frames, poses, P, viewing_cos_limit, log_scale_factor, th, nn_ratio, far_points, th_far_points, frustum,
                         n_to_match, assign, n_matches, false);
}

int ft_tracked_batch_wait(ft_tracked_batch *tb) {
    FT_REQUIRE(tb, "ft_tracked_batch_wait: null batch");
    std::lock_guard<std::mutex> lk(tb->mu);
    return waitCall(tb);
}

// the blocking forms: submit + wait
int ft_tracked_batch_search_last_frame(ft_tracked_batch *tb, int n_frames, const ft_last_points *L, const float *Tcw, float th,
                                       const int *forward, const int *backward, int check_orientation, int *const *assign,
                                       int *n_matches) {
    return searchLastMatrices(tb, n_frames, L, Tcw, th, forward, backward, check_orientation, assign, n_matches, true);
}

int ft_tracked_batch_search_last_frame_se3(ft_tracked_batch *tb, int n_frames, const ft_last_points *L, const ft_se3 *Tcw,
                                           const ft_se3 *Trl, float th, const int *forward, const int *backward,
                                           int check_orientation, int *const *assign, int *n_matches) {
    return searchLastSe3(tb, n_frames, L, Tcw, Trl, th, forward, backward, check_orientation, assign, n_matches, true);
}

int ft_tracked_batch_track_local_map(ft_tracked_batch *tb, int n_frames, const ft_frame_pose *poses, const ft_map_points *P,
                                     float viewing_cos_limit, float log_scale_factor, float th, float nn_ratio, int far_points,
                                     float th_far_points, const ft_frustum_result *frustum, int *n_to_match, int *const *assign,
                                     int *n_matches) {
    return trackLocalMap(tb, n_frames, poses, P, viewing_cos_limit, log_scale_factor, th, nn_ratio, far_points, th_far_points, frustum,
                         n_to_match, assign, n_matches, true);
}

int ft_tracked_batch_bind_fisheye(ft_tracked_batch *tb, ft_extractor *exL, ft_extractor *exR, int slot0, int n_frames, int lap_l0,
                                  int lap_l1, int lap_r0, int lap_r1, const ft_frame_view *meta, const ft_fisheye_rig *rig,
                                  const float *level_sigma2, int *const *left_to_right, int *const *right_to_left, float *const *depth,
                                  float *const *p3d, int *n_stereo) {
    return ft_tracked_batch_bind_fisheye_slots(tb, exL, exR, slot0, slot0, n_frames, lap_l0, lap_l1, lap_r0, lap_r1, meta, rig, level_sigma2,
                                               left_to_right, right_to_left, depth, p3d, n_stereo);
}

int ft_tracked_batch_bind_fisheye_slots(ft_tracked_batch *tb, ft_extractor *exL, ft_extractor *exR, int slot0, int slot0_right,
                                        int n_frames, int lap_l0, int lap_l1, int lap_r0, int lap_r1, const ft_frame_view *meta,
                                        const ft_fisheye_rig *rig, const float *level_sigma2, int *const *left_to_right,
                                        int *const *right_to_left, float *const *depth, float *const *p3d, int *n_stereo) {
    FT_REQUIRE(tb && exL && exR && meta && n_frames > 0 && n_frames <= tb->maxFrames && slot0 >= 0 && slot0_right >= 0,
               "ft_tracked_batch_bind_fisheye: bad argument");
    FT_REQUIRE(exL->ctx == tb->ctx && exR->ctx == tb->ctx, "ft_tracked_batch_bind_fisheye: extractors of another context");
    FT_REQUIRE(slot0 + n_frames <= exL->lastBatch && slot0_right + n_frames <= exR->lastBatch,
               "ft_tracked_batch_bind_fisheye: the extractors' last batches hold fewer images");
    FT_REQUIRE(exL != exR || slot0 + n_frames <= slot0_right || slot0_right + n_frames <= slot0,
               "ft_tracked_batch_bind_fisheye: one extractor for both cameras needs disjoint slot ranges");
    FT_REQUIRE(!rig || level_sigma2, "ft_tracked_batch_bind_fisheye: a rig needs level_sigma2 (mvLevelSigma2)");
    FT_REQUIRE((!depth && !p3d && !n_stereo) || rig, "ft_tracked_batch_bind_fisheye: depth / p3d / n_stereo come from the triangulation: pass a rig");
    FT_REQUIRE(!depth == !p3d, "ft_tracked_batch_bind_fisheye: depth and p3d go together");
    int nlevelsMax = 1, maxKp = 1;
    for (int f = 0; f < n_frames; f++) {
        const ft_frame_view &F = meta[f];
        FT_REQUIRE(F.Nleft >= 0 && F.N >= F.Nleft && F.N <= tb->maxKp, "ft_tracked_batch_bind_fisheye: keypoint counts out of range");
        FT_REQUIRE(F.Nleft == exL->h_nSel[slot0 + f] && F.N - F.Nleft == exR->h_nSel[slot0_right + f],
                   "ft_tracked_batch_bind_fisheye: meta's keypoint counts differ from the extractors' slots");
        FT_REQUIRE(F.scale_factors && F.nlevels >= 1 && F.nlevels <= FT_MAX_LEVELS, "scale factors missing");
        FT_REQUIRE(F.cam_model == 0 || F.cam_model == 1, "unknown camera model");
        nlevelsMax = std::max(nlevelsMax, F.nlevels);
        maxKp = std::max(maxKp, F.Nleft);
    }
    ft_context *ctx = tb->ctx;
    int rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(tb->mu);
    FT_REQUIRE(tb->call.kind == 0, "ft_tracked_batch_bind_fisheye: a submitted search of this batch has not been waited for (ft_tracked_batch_wait)");
    FtTimer tAll;
    hipStream_t st = tb->stream;
    bool wantGrid;
    {
        std::lock_guard<std::mutex> lo(ctx->matchMutex);
        wantGrid = ctx->tuning.search_grid != 0;
    }
    tb->hasGrid = false;
    FT_HIP(hipStreamSynchronize(st));
    // frames region: holder_obs of all frames, the (monoLeft, monoRight) counts, then every frame's arrays (as ft_tracked_batch_upload)
    Arena a;
    tb->holderOff.assign(n_frames, 0);
    tb->holderBegin = a.off;
    for (int f = 0; f < n_frames; f++) tb->holderOff[f] = a.take(sizeof(int) * std::max(meta[f].N, 1));
    tb->holderEnd = a.off;
    const size_t oMono = a.take(sizeof(int) * 2 * (size_t)n_frames);
    const size_t oNst = a.take(sizeof(int) * (size_t)n_frames);
    struct Lay {
        size_t keys, keysR, desc, l2r, r2l, depth, p3d;
    };
    std::vector<Lay> lay(n_frames);
    for (int f = 0; f < n_frames; f++) {
        const int nL = meta[f].Nleft, nR = meta[f].N - nL;
        lay[f].keys = a.take(sizeof(ft_keypoint) * std::max(nL, 1));
        lay[f].keysR = a.take(sizeof(ft_keypoint) * std::max(nR, 1));
        lay[f].desc = a.take((size_t)32 * std::max(meta[f].N, 1));
        lay[f].l2r = a.take(sizeof(int) * std::max(nL, 1));
        lay[f].r2l = a.take(sizeof(int) * std::max(nR, 1));
        lay[f].depth = depth ? a.take(sizeof(float) * std::max(nL, 1)) : 0;   // (inside the uright / slack share of the frame's budget)
        lay[f].p3d = depth ? a.take(3 * sizeof(float) * std::max(nL, 1)) : 0;
    }
    FT_REQUIRE(a.off <= tb->framesBytes, "ft_tracked_batch_bind_fisheye: frames region too small");
    const bool wantTables = left_to_right && right_to_left;
    const bool wantOut = wantTables || depth || n_stereo;
    Arena o;
    std::vector<size_t> outL(n_frames), outR(n_frames), outD(n_frames), outP(n_frames);
    const size_t outN = o.take(sizeof(int) * (size_t)n_frames);
    for (int f = 0; f < n_frames; f++) {
        if (wantTables) {
            outL[f] = o.take(sizeof(int) * std::max(meta[f].Nleft, 1));
            outR[f] = o.take(sizeof(int) * std::max(meta[f].N - meta[f].Nleft, 1));
        }
        if (depth) {
            outD[f] = o.take(sizeof(float) * std::max(meta[f].Nleft, 1));
            outP[f] = o.take(3 * sizeof(float) * std::max(meta[f].Nleft, 1));
        }
    }
    FT_REQUIRE(o.off <= tb->outBytes, "ft_tracked_batch_bind_fisheye: result buffer too small");
    tb->nFrames = n_frames;
    tb->DF.assign(n_frames, FtDevFrame());
    uint8_t *pinF = tb->h_in + tb->workBytes, *devF = tb->d_arena + tb->oFrames;
    FtBatchJob *hJobs = (FtBatchJob *)tb->h_in;
    FtDeliverRec *hRecs = (FtDeliverRec *)(tb->h_in + (((size_t)n_frames * sizeof(FtBatchJob) + 63) & ~(size_t)63));
    // records per frame: l2r, r2l, depth, p3d (unused ones have 0 words); then the match counts; then the two tables of depth /
    // p3d pointers the triangulation kernel reads
    const int nRecs = 4 * n_frames + 1;
    float **hDepthTab = (float **)(hRecs + nRecs), **hP3dTab = hDepthTab + n_frames;
    const size_t headBytes = (size_t)((uint8_t *)(hP3dTab + n_frames) - tb->h_in);
    FT_REQUIRE(headBytes <= tb->workBytes, "ft_tracked_batch_bind_fisheye: work region too small");
    const std::function<void(int, int)> stage = [&](int f, int) {
        const ft_frame_view &F = meta[f];
        const int nL = F.Nleft, nR = F.N - nL;
        int *hold = (int *)(pinF + tb->holderOff[f]);
        for (int i = 0; i < F.N; i++) hold[i] = F.holder_obs ? F.holder_obs[i] : -1;
        FtDevFrame &D = tb->DF[f];
        D = devFrameConstants(&F);
        D.keys = (const ft_keypoint *)(devF + lay[f].keys);
        D.keysR = (const ft_keypoint *)(devF + lay[f].keysR);
        D.desc = devF + lay[f].desc;
        D.uright = nullptr;
        D.holderObs = (const int *)(devF + tb->holderOff[f]);
        D.l2r = (const int *)(devF + lay[f].l2r);
        D.r2l = (const int *)(devF + lay[f].r2l);
        if (wantGrid) pointGrid(D, (int *)(tb->d_arena + tb->oGrid + (size_t)f * tb->gridStride));
        memset(&hJobs[f], 0, sizeof(FtBatchJob));
        hJobs[f].F = D;
        FtDeliverRec *R = hRecs + 4 * (size_t)f;
        memset(R, 0, 4 * sizeof(FtDeliverRec));
        if (wantTables) {
            R[0].dst = tb->h_out + outL[f];
            R[0].src[0] = R[0].src[1] = D.l2r;
            R[0].words = nL;
            R[1].dst = tb->h_out + outR[f];
            R[1].src[0] = R[1].src[1] = D.r2l;
            R[1].words = nR;
        }
        hDepthTab[f] = hP3dTab[f] = nullptr;
        if (depth) {
            hDepthTab[f] = (float *)(devF + lay[f].depth);
            hP3dTab[f] = (float *)(devF + lay[f].p3d);
            R[2].dst = tb->h_out + outD[f];
            R[2].src[0] = R[2].src[1] = hDepthTab[f];
            R[2].words = nL;
            R[3].dst = tb->h_out + outP[f];
            R[3].src[0] = R[3].src[1] = hP3dTab[f];
            R[3].words = 3 * nL;
        }
    };
    ctx->pool->parallel_for(n_frames, stage);
    hRecs[4 * (size_t)n_frames].dst = tb->h_out + outN;
    hRecs[4 * (size_t)n_frames].src[0] = hRecs[4 * (size_t)n_frames].src[1] = devF + oNst;
    hRecs[4 * (size_t)n_frames].words = n_frames;
    FT_HIP(hipMemcpyAsync(tb->d_arena + tb->oWork, tb->h_in, headBytes, hipMemcpyHostToDevice, st));
    if (tb->holderEnd > tb->holderBegin)
        FT_HIP(hipMemcpyAsync(devF + tb->holderBegin, pinF + tb->holderBegin, tb->holderEnd - tb->holderBegin, hipMemcpyHostToDevice, st));
    FT_HIP(hipEventRecord(tb->evMirror, st));
    const FtBatchJob *dJobs = (const FtBatchJob *)(tb->d_arena + tb->oWork);
    FtBindArgs A;
    A.keysL = exL->d_keys; A.keysR = exR->d_keys;
    A.descL = exL->d_desc; A.descR = exR->d_desc;
    A.strideL = exL->geom.maxKp; A.strideR = exR->geom.maxKp;
    A.slot0L = slot0;
    A.slot0R = slot0_right;
    A.lapL0 = lap_l0; A.lapL1 = lap_l1; A.lapR0 = lap_r0; A.lapR1 = lap_r1;
    A.mono = (int *)(devF + oMono);
    A.triangulate = rig ? 1 : 0;
    memset(&A.rig, 0, sizeof A.rig);
    if (rig) {
        memcpy(A.rig.cam1, rig->cam1, sizeof A.rig.cam1);
        memcpy(A.rig.cam2, rig->cam2, sizeof A.rig.cam2);
        A.rig.precision = rig->precision;
        memcpy(A.rig.Rlr, rig->Rlr, sizeof A.rig.Rlr);
        memcpy(A.rig.tlr, rig->tlr, sizeof A.rig.tlr);
        for (int i = 0; i < nlevelsMax; i++) A.rig.sigma2[i] = level_sigma2[i];
    }
    A.nMatches = (int *)(devF + oNst);
    const uint8_t *dWork = tb->d_arena + tb->oWork;
    A.depth = depth ? (float *const *)(dWork + ((uint8_t *)hDepthTab - tb->h_in)) : nullptr;
    A.p3d = depth ? (float *const *)(dWork + ((uint8_t *)hP3dTab - tb->h_in)) : nullptr;
    tb->evt.begin(ctx->kernelTiming, "kernel.lap_gather+fisheye_2nn_batch", st);
    rc = ft_launch_bind_fisheye_batch(st, tb->d_arena, dJobs, n_frames, maxKp, A);
    tb->evt.end(ctx->kernelTiming, st);
    if (rc == FT_OK && rig) {
        tb->evt.begin(ctx->kernelTiming, "kernel.fisheye_triangulate_batch", st);
        rc = ft_launch_fisheye_triangulate_batch(st, tb->d_arena, dJobs, n_frames, maxKp, A);
        tb->evt.end(ctx->kernelTiming, st);
    }
    if (rc != FT_OK) return rc;
    // the extractors' slots have been read: their next batch (which overwrites them) is ordered behind this point - the call may
    // return before the gather has run (no outputs asked for), and nothing else ties the extractors' streams to this one
    FT_HIP(hipEventRecord(tb->evGather, st));
    exL->foreignReader = tb->evGather;
    exR->foreignReader = tb->evGather;
    tb->evt.begin(ctx->kernelTiming, "kernel.build_grid_batch", st);
    if (rc == FT_OK && wantGrid) {
        rc = ft_launch_build_grid_batch(st, tb->d_arena, dJobs, n_frames, nlevelsMax, true);
        if (rc == FT_OK) tb->hasGrid = true;
    }
    tb->evt.end(ctx->kernelTiming, st);
    if (rc != FT_OK) return rc;
    if (wantOut) {
        const FtDeliverRec *dRecs = (const FtDeliverRec *)(tb->d_arena + tb->oWork + ((uint8_t *)hRecs - tb->h_in));
        rc = ft_launch_deliver_batch(st, dRecs, nRecs, 3 * maxKp, 0);
        if (rc != FT_OK) return rc;
        FT_HIP(hipStreamSynchronize(st));
        for (int f = 0; f < n_frames; f++) {
            const int nL = meta[f].Nleft, nR = meta[f].N - nL;
            if (wantTables && left_to_right[f] && nL) memcpy(left_to_right[f], tb->h_out + outL[f], sizeof(int) * nL);
            if (wantTables && right_to_left[f] && nR) memcpy(right_to_left[f], tb->h_out + outR[f], sizeof(int) * nR);
            if (depth && depth[f] && nL) memcpy(depth[f], tb->h_out + outD[f], sizeof(float) * nL);
            if (depth && p3d[f] && nL) memcpy(p3d[f], tb->h_out + outP[f], 3 * sizeof(float) * nL);
            if (n_stereo) n_stereo[f] = ((const int *)(tb->h_out + outN))[f];
        }
    }
    ctx->addStat("tracked_batch.bind_fisheye.total", tAll.ms());
    return FT_OK;
}

}  // extern "C"

// Host side of the rectified stereo matcher: ft_stereo_match replaces KernelController::launchStereoMatchKernel (reference
// include/Kernels/KernelController.h:31-36), and the ft_stereo_frontend_* calls offer the fused extract+match front end used
// for throughput.  Everything here lives on the streams of the two extractors (ft_host.h), nothing on the call skeleton of the
// one-shot calls.  The match itself is in kernels_stereo.hip, the delivery of a small batch in kernels_frontend_io.hip.
#include <algorithm>
#include <cstring>
#include <memory>

#include "ft_host.h"

#define FT_GRAPH_MAX_BATCH 8  // latency mode: batches up to this size are captured as graphs / run paired

static bool sameGeometry(const ft_extractor *a, const ft_extractor *b) {
    return a->width == b->width && a->height == b->height && a->nlevels == b->nlevels &&
           a->scaleFactor == b->scaleFactor && a->ctx == b->ctx;
}

// one camera's input of the stereo match (device): keypoints, descriptors (n x 32), count(s)
struct StereoSide {
    const ft_keypoint *keys;
    const uint8_t *desc;
    const int *n;
};
// FtStereoArgs from the two cameras' arrays (`capacity` records between images), the outputs, the row buffers and the rig
static FtStereoArgs stereoArgs(StereoSide l, StereoSide r, int capacity, float *uright, float *depth, int *sad, int *hamIdx, int *nMatches,
                               int medianCut, int *rowStart, int rowStride, FtSortedR *sorted, int *leftOrder, float mbf, float mb,
                               bool aligned) {
    FtStereoArgs a{};
    a.keysL = l.keys;
    a.keysR = r.keys;
    a.descL = l.desc;
    a.descR = r.desc;
    a.nL = l.n;
    a.nR = r.n;
    a.capacity = capacity;
    a.mbf = mbf;
    a.mb = mb;
    a.uright = uright;
    a.depth = depth;
    a.sad = sad;
    a.hamIdx = hamIdx;
    a.nMatches = nMatches;
    a.applyMedianCut = medianCut;
    a.rowStart = rowStart;
    a.sorted = sorted;
    a.rowStride = rowStride;
    a.leftOrder = leftOrder;
    a.alignedLoads = aligned;
    return a;
}

// ft_stereo_match's device scratch for C keypoints per camera: one allocation, every array 256 bytes aligned
struct StereoScratch {
    size_t keys, desc, out, ints, sorted, total = 0;
    StereoScratch(int C, int height) {
        auto take = [&](size_t bytes) {
            const size_t o = total;
            total = (total + bytes + 255) & ~(size_t)255;
            return o;
        };
        keys = take(sizeof(ft_keypoint) * 2 * C);  // left then right
        desc = take((size_t)64 * C);
        out = take(sizeof(float) * 2 * C);  // uright then depth
        // sad, hamming idx, then nL nR nMatches (+ pad), then the row starts, then the left order
        ints = take(sizeof(int) * (3 * (size_t)C + 8 + height + 2));
        sorted = take(sizeof(FtSortedR) * (size_t)C);  // right keypoints in row-bucket order
    }
};

extern "C" {

int ft_stereo_match(ft_extractor *exL, ft_extractor *exR, int slot, const ft_keypoint *keysL, int nL,
                    const ft_keypoint *keysR, int nR, const uint8_t *descL, const uint8_t *descR, float mbf,
                    float mb, int apply_median_cut, float *uright, float *depth, int *sad, int *n_matches) {
    FT_REQUIRE(exL && exR && uright && depth, "ft_stereo_match: null argument");
    FT_REQUIRE(sameGeometry(exL, exR), "ft_stereo_match: extractors differ in geometry or context");
    FT_REQUIRE(slot >= 0 && slot < exL->lastBatch && slot < exR->lastBatch, "ft_stereo_match: slot holds no pyramid");
    FT_REQUIRE(nL >= 0 && nR >= 0 && nL < 65536 && nR < 65536, "ft_stereo_match: keypoint count out of range");
    FT_REQUIRE(nL == 0 || (keysL && descL), "ft_stereo_match: null left arrays");
    FT_REQUIRE(nR == 0 || (keysR && descR), "ft_stereo_match: null right arrays");
    int rc = ft_set_device(exL->ctx);
    if (rc != FT_OK) return rc;
    if (nL == 0) {
        if (n_matches) *n_matches = 0;
        return FT_OK;
    }
    const int cap = std::max(std::max(nL, nR), 1);
    const FtGeom &g = exL->geom;
    static_assert(sizeof(ft_keypoint) == 28, "ft_keypoint must match cv::KeyPoint");
    // device scratch for the host arrays: grows to the largest request
    const int need = std::max(cap, g.maxKp);
    if (need > exL->stCap) {
        exL->own.giveBack(exL->d_stScratch);
        exL->stCap = 0;
        FT_CHECK(exL->own.devAlloc(&exL->d_stScratch, StereoScratch(need, exL->height).total));
        exL->stCap = need;
    }
    const int C = exL->stCap;
    const StereoScratch o(C, exL->height);
    ft_keypoint *dKeys = (ft_keypoint *)(exL->d_stScratch + o.keys);
    uint8_t *dDesc = exL->d_stScratch + o.desc;
    float *dOut = (float *)(exL->d_stScratch + o.out);
    int *dInt = (int *)(exL->d_stScratch + o.ints), *d_hdr = dInt + 2 * C;
    hipStream_t st = exL->stream;
    FT_HIP(hipStreamSynchronize(exR->stream));  // right pyramid must be complete
    FT_HIP(hipStreamSynchronize(exR->streamB));
    FT_HIP(hipStreamSynchronize(exL->streamB));
    FT_HIP(hipMemcpyAsync(dKeys, keysL, sizeof(ft_keypoint) * nL, hipMemcpyHostToDevice, st));
    FT_HIP(hipMemcpyAsync(dDesc, descL, (size_t)32 * nL, hipMemcpyHostToDevice, st));
    if (nR > 0) {
        FT_HIP(hipMemcpyAsync(dKeys + C, keysR, sizeof(ft_keypoint) * nR, hipMemcpyHostToDevice, st));
        FT_HIP(hipMemcpyAsync(dDesc + (size_t)32 * C, descR, (size_t)32 * nR, hipMemcpyHostToDevice, st));
    }
    const int hdr[4] = {nL, nR, 0, 0};
    FT_HIP(hipMemcpyAsync(d_hdr, hdr, sizeof hdr, hipMemcpyHostToDevice, st));
    // (capacity C: a single pair, the stride is irrelevant but bounds the grid)
    FtStereoArgs a = stereoArgs({dKeys, dDesc, d_hdr}, {dKeys + C, dDesc + (size_t)32 * C, d_hdr + 1}, C, dOut, dOut + C, dInt, dInt + C,
                                d_hdr + 2, apply_median_cut, d_hdr + 4, exL->height + 2, (FtSortedR *)(exL->d_stScratch + o.sorted),
                                d_hdr + 4 + exL->height + 2, mbf, mb, exL->l0Aligned && exR->l0Aligned);
    FT_CHECK(ft_launch_stereo_rowsort(st, g, 1, a));
    FT_CHECK(ft_launch_stereo_match(st, g, 1, exL->d_l0 + slot, exR->d_l0 + slot, exL->l0pitch, exR->l0pitch,
                                    exL->d_pyr + (size_t)slot * g.pyrPerSlot, exR->d_pyr + (size_t)slot * g.pyrPerSlot, a));
    FT_CHECK(ft_launch_stereo_median(st, 1, a));
    FT_HIP(hipMemcpyAsync(uright, a.uright, sizeof(float) * nL, hipMemcpyDeviceToHost, st));
    FT_HIP(hipMemcpyAsync(depth, a.depth, sizeof(float) * nL, hipMemcpyDeviceToHost, st));
    if (sad) FT_HIP(hipMemcpyAsync(sad, a.sad, sizeof(int) * nL, hipMemcpyDeviceToHost, st));
    int nm = 0;
    FT_HIP(hipMemcpyAsync(&nm, a.nMatches, sizeof(int), hipMemcpyDeviceToHost, st));
    FT_HIP(hipStreamSynchronize(st));
    if (n_matches) *n_matches = nm;
    return FT_OK;
}

// ---- fused front end ---------------------------------------------------------------------------
int ft_stereo_frontend_create(ft_context *ctx, int nfeatures, float scale_factor, int nlevels, int ini_th_fast,
                              int min_th_fast, int image_width, int image_height, int max_batch, float mbf, float mb,
                              ft_stereo_frontend **out) {
    FT_REQUIRE(ctx && out, "ft_stereo_frontend_create: null argument");
    *out = nullptr;
    ft_stereo_frontend *fe = new ft_stereo_frontend();
    std::unique_ptr<ft_stereo_frontend, int (*)(ft_stereo_frontend *)> guard(fe, ft_stereo_frontend_destroy);  // (any early return)
    fe->ctx = ctx;
    fe->mbf = mbf;
    fe->mb = mb;
    fe->maxBatch = max_batch;
    const bool pairedOn = ctx->tuning.paired != 0;
    fe->pairedCapable = pairedOn && max_batch >= 1 && max_batch <= FT_GRAPH_MAX_BATCH;
    FT_CHECK(ft_extractor_create(ctx, nfeatures, scale_factor, nlevels, ini_th_fast, min_th_fast, image_width, image_height,
                                 fe->pairedCapable ? 2 * max_batch : max_batch, &fe->exL));
    FT_CHECK(ft_extractor_create(ctx, nfeatures, scale_factor, nlevels, ini_th_fast, min_th_fast, image_width, image_height,
                                 max_batch, &fe->exR));
    fe->capacity = fe->exL->geom.maxKp;
    const size_t n = (size_t)max_batch * fe->capacity;
    FtOwned &own = fe->own;
    FT_CHECK(own.devAlloc(&fe->d_uright, n));
    FT_CHECK(own.devAlloc(&fe->d_depth, n));
    FT_CHECK(own.devAlloc(&fe->d_sad, n));
    FT_CHECK(own.devAlloc(&fe->d_nMatches, max_batch));
    FT_CHECK(own.devAlloc(&fe->d_sorted, n));
    FT_CHECK(own.devAlloc(&fe->d_rowStart, (size_t)max_batch * (image_height + 2)));
    FT_CHECK(own.devAlloc(&fe->d_leftOrder, n));
    FT_CHECK(own.pinAlloc(&fe->h_uright, n));
    FT_CHECK(own.pinAlloc(&fe->h_depth, n));
    FT_CHECK(own.pinAlloc(&fe->h_nMatches, max_batch));
    FT_CHECK(own.event(&fe->evFork));
    FT_CHECK(own.event(&fe->evJoin));
    for (int i = 0; i < 2; i++) FT_CHECK(own.event(&fe->evDone[i]));
    *out = guard.release();
    return FT_OK;
}

int ft_stereo_frontend_destroy(ft_stereo_frontend *fe) {
    if (!fe) return FT_OK;
    hipSetDevice(fe->ctx->device);
    ft_extractor_destroy(fe->exL);
    ft_extractor_destroy(fe->exR);
    if (fe->graphExec) hipGraphExecDestroy(fe->graphExec);
    fe->own.release();
    delete fe;
    return FT_OK;
}

ft_extractor *ft_stereo_frontend_left(ft_stereo_frontend *fe) { return fe ? fe->exL : nullptr; }
ft_extractor *ft_stereo_frontend_right(ft_stereo_frontend *fe) { return fe ? fe->exR : nullptr; }

// The front end's match from slot b0 on: the left camera in the left extractor's arrays, the right one in `r` - the right
// extractor's, or the upper half of the left extractor's in a paired batch.
static FtStereoArgs frontendStereoArgs(const ft_stereo_frontend *fe, int b0, StereoSide r, bool aligned) {
    const ft_extractor *L = fe->exL;
    const int maxKp = L->geom.maxKp, rowStride = L->height + 2;
    const size_t o = (size_t)b0 * maxKp;
    return stereoArgs({L->d_keys + o, L->d_desc + o * 32, L->d_nSel + b0}, r, maxKp, fe->d_uright + o, fe->d_depth + o, fe->d_sad + o,
                      nullptr, fe->d_nMatches + b0, 1, fe->d_rowStart + (size_t)b0 * rowStride, rowStride, fe->d_sorted + o,
                      fe->d_leftOrder + o, fe->mbf, fe->mb, aligned);
}
// Delivery of a whole small batch by one kernel: `r` and `overflowR` as above; the host side of the right camera is always
// the right extractor's (in a paired batch it only lends its pinned staging and counters).  direct: the rows go to the
// caller's pinned arrays (`capacity` records per image) instead of the staging.
static FtDeliverArgs frontendDeliverArgs(const ft_stereo_frontend *fe, StereoSide r, const int *overflowR, bool direct, ft_keypoint *keysL,
                                         uint8_t *descL, ft_keypoint *keysR, uint8_t *descR, float *uright, float *depth, int capacity) {
    const ft_extractor *L = fe->exL, *R = fe->exR;
    FtDeliverArgs d = ft_deliver_args(L);
    d.keysR = r.keys;
    d.descR = r.desc;
    d.nR = r.n;
    d.overflowR = overflowR;
    d.uright = fe->d_uright;
    d.depth = fe->d_depth;
    d.nMatches = fe->d_nMatches;
    if (direct) {
        d.oKeysL = keysL;
        d.oDescL = descL;
        d.dstStride = capacity;
    }
    d.oKeysR = direct ? keysR : R->h_keys;
    d.oDescR = direct ? descR : R->h_desc;
    d.oUright = direct ? uright : fe->h_uright;
    d.oDepth = direct ? depth : fe->h_depth;
    d.oNR = R->h_nSel;
    d.oNMatches = fe->h_nMatches;
    d.oOverflowR = R->h_overflow;
    return d;
}

// Matching and result copies of the slots [b0, b0 + nb) once their descriptors are enqueued on the stage-B streams of the
// two extractors: row sort, stereo match, median cut on the left stage-B stream, then (unless one kernel delivers the whole
// batch at the end) the D2H copies of the rows.  Also the tail of the per-image host-octree repair.
static int frontendMatchAndDeliver(ft_stereo_frontend *fe, int s, int b0, int nb, bool dev, bool deliver, bool direct,
                                   ft_keypoint *keysL, uint8_t *descL, ft_keypoint *keysR, uint8_t *descR, int capacity,
                                   float *uright, float *depth) {
    ft_extractor *L = fe->exL, *R = fe->exR;
    const FtGeom &g = L->geom;
    const bool tm = fe->ctx->kernelTiming;
    hipStream_t st = L->streamB;
    int rc;
    // pageable result arrays go through the library's pinned staging buffers and a host memcpy in _wait
    // (with the device octree the per-image counts are unknown until the end: whole rows are copied, which the
    // caller's arrays must be able to hold)
    const size_t kp = sizeof(ft_keypoint);
    auto d2h = [&](void *user, void *staging, const void *dev, size_t elem, int b0, int nb, int maxN) -> hipError_t {
        // rows of `elem`-byte records: device/staging stride maxKp, user stride capacity
        const size_t o = (size_t)b0 * g.maxKp * elem;
        if (direct) {
            if (!user) return hipSuccess;
            return hipMemcpy2DAsync((uint8_t *)user + (size_t)b0 * capacity * elem, elem * capacity, (const uint8_t *)dev + o,
                                    elem * g.maxKp, elem * maxN, nb, hipMemcpyDeviceToHost, st);
        }
        return hipMemcpy2DAsync((uint8_t *)staging + o, elem * g.maxKp, (const uint8_t *)dev + o, elem * g.maxKp, elem * maxN,
                                nb, hipMemcpyDeviceToHost, st);
    };
    FT_HIP(hipEventRecord(R->evB[s], R->streamB));
    FT_HIP(hipStreamWaitEvent(st, R->evB[s], 0));
    // keypoints stay on the device between extraction and matching: pinhole stereo passes the lapping
    // area (0,0) (src/Frame.cc:127), no keypoint has x == 0, so mono order == extraction order.
    const size_t o = (size_t)b0 * g.maxKp;
    const FtStereoArgs a = frontendStereoArgs(fe, b0, {R->d_keys + o, R->d_desc + o * 32, R->d_nSel + b0}, L->l0Aligned && R->l0Aligned);
    L->evt.begin(tm, "kernel.stereo_rowsort", st);
    rc = ft_launch_stereo_rowsort(st, g, nb, a);
    L->evt.end(tm, st);
    if (rc != FT_OK) return rc;
    L->evt.begin(tm, "kernel.stereo_match", st);
    rc = ft_launch_stereo_match(st, g, nb, L->d_l0 + b0, R->d_l0 + b0, L->l0pitch, R->l0pitch,
                                L->d_pyr + (size_t)b0 * g.pyrPerSlot, R->d_pyr + (size_t)b0 * g.pyrPerSlot, a);
    L->evt.end(tm, st);
    if (rc != FT_OK) return rc;
    L->evt.begin(tm, "kernel.stereo_median", st);
    rc = ft_launch_stereo_median(st, nb, a);
    L->evt.end(tm, st);
    if (rc != FT_OK) return rc;
    int maxNL = 0, maxNR = 0;
    for (int b = b0; b < b0 + nb; b++) {
        maxNL = std::max(maxNL, dev ? g.maxKp : L->h_nSel[b]);
        maxNR = std::max(maxNR, dev ? g.maxKp : R->h_nSel[b]);
    }
    if (!dev && (maxNL > capacity || maxNR > capacity)) {
        ft_set_error("stereo front end: output capacity too small (use ft_extractor_max_keypoints)");
        return FT_ERR_CAPACITY;
    }
    if (deliver) return FT_OK;  // one kernel at the end delivers everything
    if (maxNL > 0) {
        FT_HIP(d2h(keysL, L->h_keys, L->d_keys, kp, b0, nb, maxNL));
        FT_HIP(d2h(descL, L->h_desc, L->d_desc, 32, b0, nb, maxNL));
        FT_HIP(d2h(uright, fe->h_uright, fe->d_uright, 4, b0, nb, maxNL));
        FT_HIP(d2h(depth, fe->h_depth, fe->d_depth, 4, b0, nb, maxNL));
    }
    if (maxNR > 0) {
        FT_HIP(d2h(keysR, R->h_keys, R->d_keys, kp, b0, nb, maxNR));
        FT_HIP(d2h(descR, R->h_desc, R->d_desc, 32, b0, nb, maxNR));
    }
    FT_HIP(hipMemcpyAsync(fe->h_nMatches + b0, fe->d_nMatches + b0, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
    return FT_OK;
}

// enqueues one batch on the front end's streams.  capture != 0: L->stream is being captured into a graph - the other
// streams are forked from it first and joined back at the end, and nothing here may synchronise.
static int frontendEnqueue(ft_stereo_frontend *fe, const uint8_t *const *imagesL, const uint8_t *const *imagesR, int batch,
                           int on_device, int width, int height, int stride, ft_keypoint *keysL, uint8_t *descL, int *nL,
                           ft_keypoint *keysR, uint8_t *descR, int *nR, int capacity, float *uright, float *depth,
                           int *n_matches, bool direct, int capture, bool paired) {
    ft_extractor *L = fe->exL, *R = fe->exR;
    const FtGeom &g = L->geom;
    FtTimer tAll;
    fe->lastPaired = paired;
    if (paired) {
        // both cameras through the left extractor: slots [0, B) left, [B, 2B) right; one launch per kernel
        const int B = batch;
        std::vector<const uint8_t *> imgs(imagesL, imagesL + B);
        imgs.insert(imgs.end(), imagesR, imagesR + B);
        FT_CHECK(ft_extract_prepare(L, imgs.data(), 2 * B, on_device, width, height, stride));
        fe->ctx->addStat("stereo.device_octree_batches", 0);
        FT_CHECK(ft_extract_launch_a(L, 0, 2 * B, nullptr));
        FT_CHECK(ft_extract_launch_octree(L, 0, 0, 2 * B, L->evA[0]));
        hipStream_t st = L->streamB;
        FT_HIP(hipStreamWaitEvent(st, L->evA[0], 0));
        FT_CHECK(ft_extract_launch_b(L, 0, 2 * B, st));
        const size_t oR = (size_t)B * g.maxKp;  // the right camera's half of the left extractor's arrays
        const StereoSide right = {L->d_keys + oR, L->d_desc + oR * 32, L->d_nSel + B};
        const FtStereoArgs a = frontendStereoArgs(fe, 0, right, L->l0Aligned);
        FT_CHECK(ft_launch_stereo_rowsort(st, g, B, a));
        FT_CHECK(ft_launch_stereo_match(st, g, B, L->d_l0, L->d_l0 + B, L->l0pitch, L->l0pitch, L->d_pyr,
                                        L->d_pyr + (size_t)B * g.pyrPerSlot, a));
        FT_CHECK(ft_launch_stereo_median(st, B, a));
        FT_CHECK(ft_launch_deliver(st, B, frontendDeliverArgs(fe, right, L->d_overflow, direct, keysL, descL, keysR, descR, uright, depth, capacity)));
        R->lastBatch = B;
        if (capture) {
            FT_HIP(hipEventRecord(fe->evJoin, st));
            FT_HIP(hipStreamWaitEvent(L->stream, fe->evJoin, 0));
        }
        fe->ctx->addStat("stereo.submit.total", tAll.ms());
        return FT_OK;
    }
    if (capture) {  // fork: everything the right camera enqueues hangs off the captured stream
        FT_HIP(hipEventRecord(fe->evFork, L->stream));
        FT_HIP(hipStreamWaitEvent(R->stream, fe->evFork, 0));
    }
    int rc = ft_extract_prepare(L, imagesL, batch, on_device, width, height, stride);
    if (rc != FT_OK) return rc;
    rc = ft_extract_prepare(R, imagesR, batch, on_device, width, height, stride);
    if (rc != FT_OK) return rc;
    // software pipeline over sub-batches: while the host distributes the keypoints of sub-batch s, the
    // GPU already runs pyramid + FAST of sub-batch s+1 (stage-A streams) and descriptors / matching of
    // sub-batch s-1 (stage-B streams)
    const int S = ft_pipeline_depth(L->tune, batch, L->deviceOctree && R->deviceOctree);
    const int sb = (batch + S - 1) / S;
    // device octree: candidates, selection and counts stay on the device, so the whole batch is enqueued
    // without a single host synchronisation; otherwise the host octree of sub-batch s runs between the stages
    const bool dev = L->deviceOctree && R->deviceOctree;
    if (!dev) L->deviceOctree = R->deviceOctree = false;
    if (dev) fe->ctx->addStat("stereo.device_octree_batches", 0);
    for (int s = 0, b0 = 0; b0 < batch; s++, b0 += sb) {
        const int nb = std::min(sb, batch - b0);
        rc = ft_extract_launch_a(L, b0, nb, dev ? nullptr : L->evA[s]);
        if (rc == FT_OK && dev) rc = ft_extract_launch_octree(L, s, b0, nb, L->evA[s]);
        if (rc != FT_OK) return rc;
        rc = ft_extract_launch_a(R, b0, nb, dev ? nullptr : R->evA[s]);
        if (rc == FT_OK && dev) rc = ft_extract_launch_octree(R, s, b0, nb, R->evA[s]);
        if (rc != FT_OK) return rc;
    }
    hipStream_t st = L->streamB;
    // latency mode: the results of a small batch are written to pinned host memory by one kernel (FtDeliverArgs); large
    // batches keep the DMA copies, which cost no compute units
    const bool deliver = dev && batch <= FT_GRAPH_MAX_BATCH;
    double tOct = 0, tWait = 0, tLaunch = 0;
    for (int s = 0, b0 = 0; b0 < batch; s++, b0 += sb) {
        const int nb = std::min(sb, batch - b0);
        if (dev) {
            FT_HIP(hipStreamWaitEvent(L->streamB, L->evA[s], 0));
            FT_HIP(hipStreamWaitEvent(R->streamB, R->evA[s], 0));
        } else {
            FtTimer tW;
            FT_HIP(hipEventSynchronize(L->evA[s]));
            FT_HIP(hipEventSynchronize(R->evA[s]));
            tWait += tW.ms();
            FtTimer tO;
            ft_extractor *both[2] = {L, R};
            rc = ft_extract_octree_multi(both, 2, b0, nb);  // one job for both cameras: one critical path
            if (rc != FT_OK) return rc;
            tOct += tO.ms();
        }
        FtTimer tL;
        rc = ft_extract_launch_b(L, b0, nb, L->streamB);
        if (rc != FT_OK) return rc;
        rc = ft_extract_launch_b(R, b0, nb, R->streamB);
        if (rc != FT_OK) return rc;
        rc = frontendMatchAndDeliver(fe, s, b0, nb, dev, deliver, direct, keysL, descL, keysR, descR, capacity, uright, depth);
        if (rc != FT_OK) return rc;
        tLaunch += tL.ms();
    }
    if (deliver) {
        FT_CHECK(ft_launch_deliver(st, batch, frontendDeliverArgs(fe, {R->d_keys, R->d_desc, R->d_nSel}, R->d_overflow, direct, keysL, descL,
                                                                  keysR, descR, uright, depth, capacity)));
    } else {
        FT_CHECK(ft_extract_finish_counts(L, batch, st));
        FT_CHECK(ft_extract_finish_counts(R, batch, st));
    }
    if (capture) {  // join: the stage-B stream of the left camera is the tail of everything
        FT_HIP(hipEventRecord(fe->evJoin, st));
        FT_HIP(hipStreamWaitEvent(L->stream, fe->evJoin, 0));
    }
    if (!dev) fe->ctx->addStat("stereo.octree(host,both)", tOct);
    fe->ctx->addStat("stereo.host_wait_stageA", tWait);
    fe->ctx->addStat("stereo.host_launch_stageB", tLaunch);
    fe->ctx->addStat("stereo.submit.total", tAll.ms());
    return FT_OK;
}

int ft_stereo_frontend_submit(ft_stereo_frontend *fe, const uint8_t *const *imagesL, const uint8_t *const *imagesR,
                              int batch, int on_device, int width, int height, int stride, ft_keypoint *keysL,
                              uint8_t *descL, int *nL, ft_keypoint *keysR, uint8_t *descR, int *nR, int capacity,
                              float *uright, float *depth, int *n_matches) {
    FT_REQUIRE(fe, "null front end");
    FT_REQUIRE(!fe->pending.active, "stereo front end: a submitted batch has not been waited for");
    if (!imagesL || !imagesR || width <= 0 || height <= 0) {
        ft_set_error("stereo front end: empty image");
        return FT_ERR_EMPTY;
    }
    ft_extractor *L = fe->exL, *R = fe->exR;
    const FtGeom &g = L->geom;
    int rc = ft_set_device(fe->ctx);
    if (rc != FT_OK) return rc;
    FT_REQUIRE(batch >= 1 && batch <= fe->maxBatch, "stereo front end: batch outside [1, max_batch]");
    rc = ft_extract_foreign_wait(L);  // (a tracked batch bound to these extractors may still read their slots; never inside a capture)
    if (rc == FT_OK) rc = ft_extract_foreign_wait(R);
    if (rc != FT_OK) return rc;
    const bool dev = L->deviceOctree && R->deviceOctree;
    const bool paired = fe->pairedCapable && dev && batch <= FT_GRAPH_MAX_BATCH && 2 * batch <= L->maxBatch;
    // result arrays in pinned host memory (ft_host_malloc) are filled by the device directly
    const bool direct = ft_is_pinned_host(keysL) && ft_is_pinned_host(descL) && ft_is_pinned_host(keysR) && ft_is_pinned_host(descR) &&
                        ft_is_pinned_host(uright) && ft_is_pinned_host(depth) && (!dev || capacity >= g.maxKp);
    // ---- latency mode: small batches with a fixed call shape run as one captured graph ----
    bool launched = false, useGraph = L->tune.graph != 0 && !fe->graphDisabled && L->ownStreams && R->ownStreams && dev && direct &&
                                      !fe->ctx->kernelTiming && batch <= FT_GRAPH_MAX_BATCH && width == L->width && height == L->height &&
                                      stride >= width;
    for (int b = 0; b < batch && useGraph; b++)
        if (!imagesL[b] || !imagesR[b]) useGraph = false;
    if (useGraph && !on_device && (ft_extract_ensure_stage(L) != FT_OK || ft_extract_ensure_stage(R) != FT_OK)) {
        (void)hipGetLastError();
        useGraph = false;
    }
    if (useGraph) {
        ft_stereo_frontend::GraphKey key;
        key.batch = batch; key.onDevice = on_device; key.width = width; key.height = height; key.stride = stride;
        key.capacity = capacity;
        key.paired = paired ? 1 : 0;
        key.bigGridL = L->bigGrid + (L->histOn ? (1 << 24) : 0);
        key.bigGridR = R->bigGrid + (R->histOn ? (1 << 24) : 0);
        key.alignedL = !on_device || ft_frames_aligned(imagesL, batch, stride);
        key.alignedR = !on_device || ft_frames_aligned(imagesR, batch, stride);
        if (paired) key.alignedL = key.alignedR = key.alignedL & key.alignedR;  // one launch reads both cameras
        const void *outs[6] = {keysL, descL, keysR, descR, uright, depth};
        for (int i = 0; i < 6; i++) key.out[i] = outs[i];
        if (fe->graphExec && key == fe->graphKey) {
            if (paired) {  // (both cameras in the left extractor: frontendEnqueue)
                std::vector<const uint8_t *> imgs(imagesL, imagesL + batch);
                imgs.insert(imgs.end(), imagesR, imagesR + batch);
                ft_extract_rebind(L, imgs.data(), 2 * batch, on_device, width, height, stride);
                R->lastBatch = batch;
            } else {
                ft_extract_rebind(L, imagesL, batch, on_device, width, height, stride);
                ft_extract_rebind(R, imagesR, batch, on_device, width, height, stride);
            }
            fe->lastPaired = paired;
            fe->ctx->addStat("stereo.device_octree_batches", 0);
            FtTimer tG;
            FT_HIP(hipGraphLaunch(fe->graphExec, L->stream));
            fe->ctx->addStat("stereo.graph_launch", tG.ms());
            launched = true;
        } else {
            L->stageHost = R->stageHost = !on_device;  // (ft_extract_prepare: host frames go through the pinned staging)
            launched = ft_graph_capture(L->stream, &fe->graphExec, [&] {
                return frontendEnqueue(fe, imagesL, imagesR, batch, on_device, width, height, stride, keysL, descL, nL, keysR, descR, nR,
                                       capacity, uright, depth, n_matches, direct, 1, paired);
            });
            L->stageHost = R->stageHost = false;
            fe->graphDisabled = !launched;  // capture is an optimisation: plain enqueueing for good
            if (launched) fe->graphKey = key;
            fe->ctx->addStat(launched ? "stereo.graph_captures" : "stereo.graph_capture_failed", 0);
            if (launched) FT_HIP(hipGraphLaunch(fe->graphExec, L->stream));
        }
    }
    if (!launched) {
        rc = frontendEnqueue(fe, imagesL, imagesR, batch, on_device, width, height, stride, keysL, descL, nL, keysR, descR,
                             nR, capacity, uright, depth, n_matches, direct, 0, paired);
        if (rc != FT_OK) return rc;
        // the end of this batch, marked NOW: ft_stereo_frontend_wait waits for these events and not for the streams - a
        // stream synchronisation enqueues its marker at the time of the call, behind whatever another front end has put
        // into the same hardware queue since (the runtime multiplexes all streams onto a few in-order queues), so waiting
        // for batch k-1 returned only when batch k was nearly through and the upload of batch k+1 started that late
        FT_HIP(hipEventRecord(fe->evDone[0], L->streamB));
        FT_HIP(hipEventRecord(fe->evDone[1], R->streamB));
    }
    // everything is enqueued; ft_stereo_frontend_wait waits for the end of the batch and finishes the outputs
    auto &P = fe->pending;
    P.imagesL.assign(imagesL, imagesL + batch);
    P.imagesR.assign(imagesR, imagesR + batch);
    P.onDevice = on_device;
    P.width = width;
    P.height = height;
    P.stride = stride;
    P.active = true;
    P.graph = launched;
    P.batch = batch;
    P.capacity = capacity;
    P.direct = direct;
    P.keysL = keysL; P.descL = descL; P.nL = nL;
    P.keysR = keysR; P.descR = descR; P.nR = nR;
    P.uright = uright; P.depth = depth; P.nMatches = n_matches;
    return FT_OK;
}

int ft_stereo_frontend_wait(ft_stereo_frontend *fe) {
    FT_REQUIRE(fe, "null front end");
    auto &P = fe->pending;
    if (!P.active) return FT_OK;
    int rc = ft_set_device(fe->ctx);
    if (rc != FT_OK) return rc;
    ft_extractor *L = fe->exL, *R = fe->exR;
    const FtGeom &g = L->geom;
    FtTimer tTail;
    P.active = false;
    if (P.graph) {
        FT_HIP(hipStreamSynchronize(L->stream));  // a captured batch completes on the stream it was launched on
        FT_HIP(hipStreamSynchronize(L->streamB));
        FT_HIP(hipStreamSynchronize(R->streamB));
    } else {
        FT_HIP(hipEventSynchronize(fe->evDone[0]));
        FT_HIP(hipEventSynchronize(fe->evDone[1]));
    }
    fe->ctx->addStat("stereo.host_tail_sync", tTail.ms());
    L->evt.resolve(fe->ctx);
    R->evt.resolve(fe->ctx);
    if (L->deviceOctree) ft_extract_update_big_grid(L);
    if (R->deviceOctree) ft_extract_update_big_grid(R);
    if ((L->deviceOctree && L->h_overflow[0]) || (R->deviceOctree && R->h_overflow[0])) {
        // a level of some image exceeded the device octree's limits (more than 16 384 candidates, or more than
        // FT_OCT_BIGCAP levels of the launch beyond 4 096)
        std::vector<int> sl, sr;
        std::vector<char> bad(P.batch, 0);
        int nBad = 0;
        if (!(P.graph || fe->lastPaired)) {
            rc = ft_extract_overflow_slots(L, P.batch, sl);
            if (rc == FT_OK) rc = ft_extract_overflow_slots(R, P.batch, sr);
            if (rc != FT_OK) return rc;
            for (int b : sl) bad[b] |= 1;
            for (int b : sr) bad[b] |= 2;
            for (int b = 0; b < P.batch; b++) nBad += bad[b] ? 1 : 0;
        }
        if (P.graph || fe->lastPaired || 4 * nBad > P.batch) {
            // latency mode (at most 8 pairs, possibly both cameras in one extractor), or most of the batch is beyond the
            // device octree: the whole batch is redone with the host-octree pipeline (sub-batches of 16 pairs, the host
            // octree of one overlapping with the kernels of the next).  Same inputs, same outputs, only slower.
            fe->ctx->addStat("stereo.device_octree_fallbacks", 1);
            for (int k = 1; k < nBad; k++) fe->ctx->addStat("stereo.device_octree_fallbacks", 1);
            L->h_overflow[0] = R->h_overflow[0] = 0;
            FT_HIP(hipMemset(L->d_overflow, 0, sizeof(int)));
            FT_HIP(hipMemset(R->d_overflow, 0, sizeof(int)));
            FT_HIP(hipMemset(L->d_ovSlot, 0, sizeof(int) * L->maxBatch));
            FT_HIP(hipMemset(R->d_ovSlot, 0, sizeof(int) * R->maxBatch));
            const bool dl = L->deviceOctree, dr = R->deviceOctree;
            L->deviceOctree = R->deviceOctree = false;
            std::vector<const uint8_t *> il = P.imagesL, ir = P.imagesR;
            rc = ft_stereo_frontend_submit(fe, il.data(), ir.data(), P.batch, P.onDevice, P.width, P.height, P.stride, P.keysL,
                                           P.descL, P.nL, P.keysR, P.descR, P.nR, P.capacity, P.uright, P.depth, P.nMatches);
            if (rc == FT_OK) rc = ft_stereo_frontend_wait(fe);
            L->deviceOctree = dl;
            R->deviceOctree = dr;
            return rc;
        }
        // throughput mode, a few pairs concerned: only they are redone, in place - host octree of the camera(s) that
        // overflowed (all of them as one parallel job), then descriptors, matching and result copies of each such pair;
        // every other pair keeps its device results
        std::vector<std::pair<ft_extractor *, int>> jobs;
        for (int b : sl) jobs.emplace_back(L, b);
        for (int b : sr) jobs.emplace_back(R, b);
        rc = ft_extract_repair_prepare(jobs);
        if (rc != FT_OK) return rc;
        for (int b = 0; b < P.batch; b++) {
            if (!bad[b]) continue;
            fe->ctx->addStat("stereo.device_octree_fallbacks", 1);
            if (bad[b] & 1) rc = ft_extract_repair_launch(L, b, L->streamB);
            if (rc == FT_OK && (bad[b] & 2)) rc = ft_extract_repair_launch(R, b, R->streamB);
            if (rc == FT_OK)
                rc = frontendMatchAndDeliver(fe, 0, b, 1, true, false, P.direct, P.keysL, P.descL, P.keysR, P.descR, P.capacity,
                                             P.uright, P.depth);
            if (rc != FT_OK) return rc;
        }
        FT_HIP(hipStreamSynchronize(L->streamB));
        FT_HIP(hipStreamSynchronize(R->streamB));
        L->evt.resolve(fe->ctx);
        R->evt.resolve(fe->ctx);
    }
    const size_t kp = sizeof(ft_keypoint);
    const int capacity = P.capacity;
    for (int b = 0; b < P.batch; b++) {
        const int nl = L->h_nSel[b], nr = R->h_nSel[b];
        if (nl > capacity || nr > capacity) {
            ft_set_error("stereo front end: output capacity too small (use ft_extractor_max_keypoints)");
            return FT_ERR_CAPACITY;
        }
        if (!P.direct) {
            if (P.keysL) memcpy(P.keysL + (size_t)b * capacity, L->h_keys + (size_t)b * g.maxKp, kp * nl);
            if (P.descL) memcpy(P.descL + (size_t)b * capacity * 32, L->h_desc + (size_t)b * g.maxKp * 32, (size_t)32 * nl);
            if (P.keysR) memcpy(P.keysR + (size_t)b * capacity, R->h_keys + (size_t)b * g.maxKp, kp * nr);
            if (P.descR) memcpy(P.descR + (size_t)b * capacity * 32, R->h_desc + (size_t)b * g.maxKp * 32, (size_t)32 * nr);
            if (P.uright) memcpy(P.uright + (size_t)b * capacity, fe->h_uright + (size_t)b * g.maxKp, 4 * (size_t)nl);
            if (P.depth) memcpy(P.depth + (size_t)b * capacity, fe->h_depth + (size_t)b * g.maxKp, 4 * (size_t)nl);
        }
        if (P.nL) P.nL[b] = nl;
        if (P.nR) P.nR[b] = nr;
        if (P.nMatches) P.nMatches[b] = fe->h_nMatches[b];
    }
    return FT_OK;
}

int ft_stereo_frontend_process(ft_stereo_frontend *fe, const uint8_t *const *imagesL, const uint8_t *const *imagesR,
                               int batch, int on_device, int width, int height, int stride, ft_keypoint *keysL,
                               uint8_t *descL, int *nL, ft_keypoint *keysR, uint8_t *descR, int *nR, int capacity,
                               float *uright, float *depth, int *n_matches) {
    FtTimer tAll;
    int rc = ft_stereo_frontend_submit(fe, imagesL, imagesR, batch, on_device, width, height, stride, keysL, descL, nL,
                                       keysR, descR, nR, capacity, uright, depth, n_matches);
    if (rc != FT_OK) return rc;
    rc = ft_stereo_frontend_wait(fe);
    if (rc == FT_OK) fe->ctx->addStat("stereo.process.total", tAll.ms());
    return rc;
}

int ft_stereo_frontend_device_descriptors(ft_stereo_frontend *fe, int slot, int right, const uint8_t **dptr, int *n) {
    FT_REQUIRE(fe && dptr && n, "ft_stereo_frontend_device_descriptors: null argument");
    ft_extractor *ex = right ? fe->exR : fe->exL;
    FT_REQUIRE(slot >= 0 && slot < fe->exR->lastBatch, "ft_stereo_frontend_device_descriptors: slot holds no result");
    // a paired batch keeps the right camera's results in the upper half of the left extractor's arrays
    const int devSlot = (right && fe->lastPaired) ? fe->exR->lastBatch + slot : slot;
    *dptr = (fe->lastPaired ? fe->exL : ex)->d_desc + (size_t)devSlot * ex->geom.maxKp * 32;
    *n = ex->h_nSel[slot];
    return FT_OK;
}

}  // extern "C"

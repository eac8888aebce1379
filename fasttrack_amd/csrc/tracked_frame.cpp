// ft_tracked_frame_*: a frame that stays on the device from its upload on (struct ft_tracked_frame: search_host.h); the
// searches stage their points only and go through the same cores as the view calls.
#include "search_host.h"

// holder_obs of the resident frame to the device, without a synchronisation: the pinned source belongs to the frame and is
// rewritten only by the next search on it, which is ordered behind this copy on the stream and synchronises the stream
// (fixedPoint) before the host gets here again
static int uploadHolder(ft_tracked_frame *tf, hipStream_t st) {
    const size_t bytes = sizeof(int) * tf->holder.size();
    if (!bytes) return FT_OK;
    memcpy(tf->h_holderUp, tf->holder.data(), bytes);
    FT_HIP(hipMemcpyAsync(tf->d_holder, tf->h_holderUp, bytes, hipMemcpyHostToDevice, st));
    return FT_OK;
}

extern "C" {

int ft_tracked_frame_create(ft_context *ctx, int max_keypoints, int max_points, ft_tracked_frame **out) {
    FT_REQUIRE(ctx && out && max_keypoints > 0 && max_points > 0, "ft_tracked_frame_create: bad argument");
    FT_REQUIRE(max_keypoints < (1 << 24) && max_points < (1 << 22), "ft_tracked_frame_create: capacity out of range");
    int rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    ft_tracked_frame *tf = new ft_tracked_frame();
    tf->ctx = ctx;
    tf->maxKp = max_keypoints;
    tf->maxPts = max_points;
    const size_t K = (size_t)max_keypoints, M = (size_t)max_points;
    // arena of one call: map points (<= 72 B) + frustum outputs (<= 48 B) + passes / raw outputs (<= 104 B) per point
    tf->workBytes = 320 * M + 112 * K + 16384;  // (108 K: list heads and writer table of the claim iteration)
    hipError_t e = hipMalloc((void **)&tf->d_keys, sizeof(ft_keypoint) * K);
    if (e == hipSuccess) e = hipMalloc((void **)&tf->d_keysR, sizeof(ft_keypoint) * K);
    if (e == hipSuccess) e = hipMalloc((void **)&tf->d_desc, 32 * K);
    if (e == hipSuccess) e = hipMalloc((void **)&tf->d_uright, sizeof(float) * K);
    if (e == hipSuccess) e = hipMalloc((void **)&tf->d_holder, sizeof(int) * K);
    if (e == hipSuccess) e = hipMalloc((void **)&tf->d_l2r, sizeof(int) * K);
    if (e == hipSuccess) e = hipMalloc((void **)&tf->d_r2l, sizeof(int) * K);
    if (e == hipSuccess) e = hipMalloc((void **)&tf->d_work, tf->workBytes);
    if (e == hipSuccess) e = hipMalloc((void **)&tf->d_grid, gridBytes((int)K));
    if (e == hipSuccess && searchCacheOn(ctx)) e = hipMalloc((void **)&tf->d_cache, searchCacheBytes(max_points));
    if (e == hipSuccess) e = hipHostMalloc((void **)&tf->h_work, tf->workBytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&tf->h_holderUp, sizeof(int) * K, hipHostMallocDefault);
    tf->frameUpBytes = (2 * sizeof(ft_keypoint) + 32 + 4 * sizeof(int)) * K + 8 * 64;
    if (e == hipSuccess) e = hipHostMalloc((void **)&tf->h_frameUp, tf->frameUpBytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        ft_tracked_frame_destroy(tf);
        return ft_hip_fail(e, "ft_tracked_frame_create", __FILE__, __LINE__);
    }
    tf->counted = true;
    ctx->liveObjects++;
    *out = tf;
    return FT_OK;
}

int ft_tracked_frame_destroy(ft_tracked_frame *tf) {
    if (!tf) return FT_OK;
    ft_set_device(tf->ctx);
    hipStreamSynchronize(tf->ctx->stream);
    hipFree(tf->d_keys); hipFree(tf->d_keysR); hipFree(tf->d_desc); hipFree(tf->d_uright);
    hipFree(tf->d_holder); hipFree(tf->d_l2r); hipFree(tf->d_r2l); hipFree(tf->d_work); hipFree(tf->d_grid);
    if (tf->d_cache) hipFree(tf->d_cache);
    if (tf->h_work) hipHostFree(tf->h_work);
    if (tf->h_holderUp) hipHostFree(tf->h_holderUp);
    if (tf->h_frameUp) hipHostFree(tf->h_frameUp);
    if (tf->d_init) hipFree(tf->d_init);
    if (tf->h_init) hipHostFree(tf->h_init);
    tf->evt.destroy();
    if (tf->counted) tf->ctx->liveObjects--;
    delete tf;
    return FT_OK;
}

int ft_tracked_frame_upload(ft_tracked_frame *tf, const ft_frame_view *F) {
    FT_REQUIRE(tf, "null tracked frame");
    int rc = checkFrame(F);
    if (rc != FT_OK) return rc;
    FT_REQUIRE(F->N <= tf->maxKp, "ft_tracked_frame_upload: more keypoints than the frame was created for");
    rc = ft_set_device(tf->ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(tf->ctx->matchMutex);
    hipStream_t st = tf->ctx->stream;
    const int nL = F->Nleft == -1 ? F->N : F->Nleft, nR = F->Nleft == -1 ? 0 : F->N - F->Nleft;
    // The caller's arrays are pageable as a rule: handed to hipMemcpyAsync as they are, each of the seven copies is staged by
    // the runtime and waited for (70 - 85 us per frame).  They are packed into the frame's own pinned buffer instead (one
    // pass of host memcpy) and go up from there as plain asynchronous copies; nothing is waited for here - the searches that
    // follow are ordered behind the copies on the stream, and the next upload waits for the stream before it repacks.
    FT_HIP(hipStreamSynchronize(st));
    {
        Arena up;
        auto put = [&](void *dst, const void *src, size_t bytes) -> int {
            if (!bytes) return FT_OK;
            const size_t o = up.take(bytes);
            memcpy(tf->h_frameUp + o, src, bytes);
            FT_HIP(hipMemcpyAsync(dst, tf->h_frameUp + o, bytes, hipMemcpyHostToDevice, st));
            return FT_OK;
        };
        if ((rc = put(tf->d_keys, F->keys, sizeof(ft_keypoint) * nL)) != FT_OK) return rc;
        if ((rc = put(tf->d_keysR, F->keys_right, sizeof(ft_keypoint) * nR)) != FT_OK) return rc;
        if ((rc = put(tf->d_desc, F->descriptors, (size_t)32 * F->N)) != FT_OK) return rc;
        if (F->uright && (rc = put(tf->d_uright, F->uright, sizeof(float) * F->N)) != FT_OK) return rc;
        if (F->Nleft != -1) {
            if ((rc = put(tf->d_l2r, F->left_to_right, sizeof(int) * nL)) != FT_OK) return rc;
            if ((rc = put(tf->d_r2l, F->right_to_left, sizeof(int) * nR)) != FT_OK) return rc;
        }
        if ((rc = put(tf->d_holder, F->holder_obs, sizeof(int) * F->N)) != FT_OK) return rc;
    }
    tf->DF = devFrameConstants(F);
    tf->DF.keys = tf->d_keys;
    tf->DF.keysR = tf->d_keysR;
    tf->DF.desc = tf->d_desc;
    tf->DF.uright = F->uright ? tf->d_uright : nullptr;
    tf->DF.holderObs = tf->d_holder;
    tf->DF.l2r = F->Nleft != -1 ? tf->d_l2r : nullptr;
    tf->DF.r2l = F->Nleft != -1 ? tf->d_r2l : nullptr;
    rc = buildGrid(tf->ctx, st, tf->DF, tf->d_grid);  // the grid of the frame, once: both searches look up their windows in it
    if (rc != FT_OK) return rc;
    tf->angles.resize(F->N);
    tf->level0 = 0;
    for (int i = 0; i < nL; i++) {
        tf->angles[i] = F->keys[i].angle;
        tf->level0 += F->keys[i].octave <= 0 ? 1 : 0;
    }
    for (int i = 0; i < nR; i++) tf->angles[nL + i] = F->keys_right[i].angle;
    tf->holder.assign(F->holder_obs, F->holder_obs + F->N);
    tf->loaded = true;
    return FT_OK;
}

int ft_tracked_frame_bind_stereo(ft_tracked_frame *tf, ft_stereo_frontend *fe, int slot, const ft_frame_view *meta) {
    FT_REQUIRE(tf && fe && meta, "ft_tracked_frame_bind_stereo: null argument");
    FT_REQUIRE(tf->ctx == fe->ctx, "tracked frame and front end belong to different contexts");
    FT_REQUIRE(!fe->pending.active, "ft_tracked_frame_bind_stereo: the front end has a submitted batch that was not waited for");
    ft_extractor *L = fe->exL;
    FT_REQUIRE(slot >= 0 && slot < fe->maxBatch, "ft_tracked_frame_bind_stereo: slot out of range");
    const int N = L->h_nSel[slot];
    FT_REQUIRE(meta->Nleft == -1, "ft_tracked_frame_bind_stereo: the stereo front end produces rectified frames (Nleft == -1)");
    FT_REQUIRE(meta->N == N, "ft_tracked_frame_bind_stereo: meta->N differs from the keypoint count of the slot");
    FT_REQUIRE(N <= tf->maxKp, "ft_tracked_frame_bind_stereo: more keypoints than the frame was created for");
    FT_REQUIRE(meta->scale_factors && meta->nlevels >= 1 && meta->nlevels <= FT_MAX_LEVELS, "scale factors missing");
    FT_REQUIRE(N == 0 || meta->keys, "ft_tracked_frame_bind_stereo: meta->keys (host copy of the keypoints) is null");
    int rc = ft_set_device(tf->ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(tf->ctx->matchMutex);
    tf->DF = devFrameConstants(meta);
    tf->DF.keys = L->d_keys + (size_t)slot * L->geom.maxKp;
    tf->DF.keysR = tf->d_keysR;
    tf->DF.desc = L->d_desc + (size_t)slot * L->geom.maxKp * 32;
    tf->DF.uright = fe->d_uright + (size_t)slot * fe->capacity;
    tf->DF.holderObs = tf->d_holder;
    tf->DF.l2r = nullptr;
    tf->DF.r2l = nullptr;
    tf->holder.assign(N, -1);
    if (meta->holder_obs) tf->holder.assign(meta->holder_obs, meta->holder_obs + N);
    tf->angles.resize(N);
    tf->level0 = 0;
    for (int i = 0; i < N; i++) {
        tf->angles[i] = meta->keys[i].angle;
        tf->level0 += meta->keys[i].octave <= 0 ? 1 : 0;
    }
    if (N) FT_HIP(hipMemcpy(tf->d_holder, tf->holder.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    rc = buildGrid(tf->ctx, tf->ctx->stream, tf->DF, tf->d_grid);  // ordered in front of the searches on the context stream
    if (rc != FT_OK) return rc;
    tf->loaded = true;
    return FT_OK;
}

int ft_tracked_frame_holder_obs(ft_tracked_frame *tf, int *holder_obs) {
    FT_REQUIRE(tf && tf->loaded && holder_obs, "ft_tracked_frame_holder_obs: no frame loaded");
    if (!tf->holder.empty()) memcpy(holder_obs, tf->holder.data(), sizeof(int) * tf->holder.size());
    return FT_OK;
}

namespace {
int trackedSearchLastFrame(ft_tracked_frame *tf, const ft_last_points *L, const FtPose &pose, const FtPose *trl, float th,
                           int forward, int backward, int check_orientation, int *assign, int *n_matches) {
    FT_REQUIRE(tf && tf->loaded && L && assign, "ft_tracked_frame_search_last_frame: null argument / no frame loaded");
    ft_context *ctx = tf->ctx;
    const int M = L->N, N = tf->DF.N;
    int rc = checkLastPoints(L, 0, tf->maxPts, "frame");
    if (rc != FT_OK) return rc;
    for (int i = 0; i < N; i++) assign[i] = -1;
    if (n_matches) *n_matches = 0;
    if (M == 0 || N == 0) return FT_OK;
    rc = checkLastPoints(L, tf->DF.nlevels, tf->maxPts, "frame");
    if (rc != FT_OK) return rc;
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    Arena a;
    const LastLayout LL = layoutLast(a, M);
    const size_t inputBytes = a.off;
    const PassLayout PL = layoutPasses(tf->ctx, a, M, N, false);
    FT_REQUIRE(a.off <= tf->workBytes, "tracked frame work arena too small");
    uint8_t *pin = tf->h_work, *dev = tf->d_work;
    stageLast(L, LL, pin);
    hipStream_t st = ctx->stream;
    FT_HIP(hipMemcpyAsync(dev, pin, inputBytes, hipMemcpyHostToDevice, st));
    FtDevFrame DF = tf->DF;
    if (trl) setTrl(DF, *trl);
    int nm = 0, passes = 0;
    rc = runLastFrameSearch(ctx, DF, devLast(M, LL, dev), passBufs(PL, dev, (const int *)(dev + LL.obs), tf->d_cache), nullptr, &tf->passesLast,
                            pose, th, forward, backward, pin, {}, L, check_orientation != 0, [&](int idx) { return tf->angles[idx]; },
                            tf->holder.data(), assign, &nm, &passes);
    if (rc != FT_OK) return rc;
    // the occupancy the next search sees: uploaded from a pinned buffer of the frame's own, so that nothing has to wait
    // for the copy (the next call on this frame is ordered behind it on the stream and synchronises before it returns)
    rc = uploadHolder(tf, st);
    if (rc != FT_OK) return rc;
    if (n_matches) *n_matches = nm;
    ctx->addStat("tracked.search_last_frame.total", tAll.ms());
    ctx->addStat("tracked.search_last_frame.passes", passes);
    return FT_OK;
}
}  // namespace

int ft_tracked_frame_search_last_frame(ft_tracked_frame *tf, const ft_last_points *L, const float *Tcw, float th,
                                       int forward, int backward, int check_orientation, int *assign, int *n_matches) {
    FT_REQUIRE(Tcw, "ft_tracked_frame_search_last_frame: null pose");
    return trackedSearchLastFrame(tf, L, poseOfMatrix(Tcw), nullptr, th, forward, backward, check_orientation, assign, n_matches);
}

int ft_tracked_frame_search_last_frame_se3(ft_tracked_frame *tf, const ft_last_points *L, const ft_se3 *Tcw, const ft_se3 *Trl,
                                           float th, int forward, int backward, int check_orientation, int *assign, int *n_matches) {
    FT_REQUIRE(tf && tf->loaded && Tcw, "ft_tracked_frame_search_last_frame_se3: null argument / no frame loaded");
    FtPose pose, trl;
    const FtPose *trlPtr = nullptr;
    const int rc = posesFromSe3(Tcw, Trl, tf->DF.Nleft != -1, "ft_tracked_frame_search_last_frame_se3", pose, trl, &trlPtr);
    if (rc != FT_OK) return rc;
    return trackedSearchLastFrame(tf, L, pose, trlPtr, th, forward, backward, check_orientation, assign, n_matches);
}

int ft_tracked_frame_track_local_map(ft_tracked_frame *tf, const ft_frame_pose *pose, const ft_map_points *P,
                                     float viewing_cos_limit, float log_scale_factor, float th, float nn_ratio,
                                     int far_points, float th_far_points, const ft_frustum_result *frustum, int *n_to_match,
                                     int *assign, int *n_matches) {
    FT_REQUIRE(tf && tf->loaded && pose && assign, "ft_tracked_frame_track_local_map: null argument / no frame loaded");
    int rc = checkMapPoints(P, true);
    if (rc != FT_OK) return rc;
    ft_context *ctx = tf->ctx;
    const int M = P->M, N = tf->DF.N;
    FT_REQUIRE(M <= tf->maxPts, "map point count beyond the frame's capacity");
    for (int i = 0; i < N; i++) assign[i] = -1;
    if (n_matches) *n_matches = 0;
    if (n_to_match) *n_to_match = 0;
    if (M == 0) return FT_OK;
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    Arena a;
    FrustumLayout FL;
    size_t fInputEnd = 0;
    layoutFrustum(M, P->skip != nullptr, a, FL, &fInputEnd);
    const size_t fOutEnd = a.off;
    const size_t oDesc = a.take(32 * (size_t)M), oObs = a.take(4 * (size_t)M);
    const PassLayout PL = layoutPasses(tf->ctx, a, M, N, false);
    FT_REQUIRE(a.off <= tf->workBytes, "tracked frame work arena too small");
    uint8_t *pin = tf->h_work, *dev = tf->d_work;
    stageFrustum(P, FL, pin);
    memcpy(pin + oDesc, P->descriptors, 32 * (size_t)M);
    memcpy(pin + oObs, P->observations, 4 * (size_t)M);
    hipStream_t st = ctx->stream;
    FT_HIP(hipMemcpyAsync(dev, pin, fInputEnd, hipMemcpyHostToDevice, st));
    FT_HIP(hipMemcpyAsync(dev + oDesc, pin + oDesc, oObs + 4 * (size_t)M - oDesc, hipMemcpyHostToDevice, st));
    const FtDevFrame DF = tf->DF;
    const FtFrustumOut FO = devFrustumOut(FL, dev);
    rc = ft_launch_frustum(st, DF, frustumPose_fromDev(DF, pose), devMapPoints(P, FL, dev), viewing_cos_limit, log_scale_factor,
                           far_points, th_far_points, FO);
    if (rc != FT_OK) return rc;
    int nm = 0, passes = 0;
    if (N > 0) {
        // the frustum fields are the search's inputs where they are: no host round trip in between; they come down with the
        // pass results (to the start of pin; the results behind them)
        rc = runLocalSearch(ctx, DF, localPointsOf(FO, M, dev + oDesc), passBufs(PL, dev, (const int *)(dev + oObs), tf->d_cache), nullptr, &tf->passesLocal, th, nn_ratio,
                            pin + fOutEnd, {pin, dev + fInputEnd, fOutEnd - fInputEnd}, P->observations, tf->holder.data(), assign, &nm,
                            &passes);
        if (rc != FT_OK) return rc;
        unpackFrustum(M, FL, fInputEnd, pin, frustum, n_to_match);
        rc = uploadHolder(tf, st);
        if (rc != FT_OK) return rc;
    } else {
        rc = downloadFrustum(st, M, FL, fInputEnd, fOutEnd, dev, pin, frustum, n_to_match);
        if (rc != FT_OK) return rc;
    }
    if (n_matches) *n_matches = nm;
    ctx->addStat("tracked.track_local_map.total", tAll.ms());
    ctx->addStat("tracked.track_local_map.passes", passes);
    return FT_OK;
}

}  // extern "C"

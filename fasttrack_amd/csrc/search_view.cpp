// The stand-alone view calls: every call stages its frame in the context's scratch arena (search_host.h has what they share
// with the resident forms).
#include "search_host.h"

extern "C" {

int ft_search_local_points(ft_context *ctx, ft_frame_view *F, const ft_local_points *P, float th, float nn_ratio,
                           int *assign, int *n_matches, int *best_dist, int *best_dist2, int *best_level,
                           int *best_level2, int *best_idx, int *best_dist_r, int *best_dist2_r, int *best_level_r,
                           int *best_level2_r, int *best_idx_r) {
    FT_REQUIRE(ctx && P && assign, "ft_search_local_points: null argument");
    int rc = checkFrame(F);
    if (rc != FT_OK) return rc;
    const int M = P->M, N = F->N;
    FT_REQUIRE(M >= 0 && M < (1 << 22), "map point count out of range");
    FT_REQUIRE(M == 0 || (P->skip && P->in_view && P->in_view_r && P->level && P->level_r && P->view_cos &&
                          P->view_cos_r && P->proj_x && P->proj_y && P->proj_xr && P->proj_yr && P->descriptors &&
                          P->observations),
               "local point arrays are null");
    for (int i = 0; i < N; i++) assign[i] = -1;
    if (n_matches) *n_matches = 0;
    int *outs[10] = {best_dist, best_dist2, best_level, best_level2, best_idx,
                     best_dist_r, best_dist2_r, best_level_r, best_level2_r, best_idx_r};
    if (M == 0 || N == 0) {
        for (int k = 0; k < 10; k++)
            if (outs[k])
                for (int i = 0; i < M; i++) outs[k][i] = (k % 5 == 0 || k % 5 == 1) ? 256 : -1;
        return FT_OK;
    }
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    // the point arrays in arena order: source, bytes per point, the device view's member (the observations: the claims')
    FtDevLocalPoints DP;
    DP.M = M;
    const int *dObs = nullptr;
    const struct {
        const void *src;
        size_t elem;
        void *dst;
    } in[13] = {{P->skip, 1, &DP.skip},        {P->in_view, 1, &DP.inView},    {P->in_view_r, 1, &DP.inViewR}, {P->level, 4, &DP.level},
                {P->level_r, 4, &DP.levelR},   {P->view_cos, 4, &DP.viewCos},  {P->view_cos_r, 4, &DP.viewCosR}, {P->proj_x, 4, &DP.projX},
                {P->proj_y, 4, &DP.projY},     {P->proj_xr, 4, &DP.projXR},    {P->proj_yr, 4, &DP.projYR},    {P->descriptors, 32, &DP.desc},
                {P->observations, 4, &dObs}};
    // ---- layout: inputs | work | outputs ----
    Arena a;
    FrameLayout FL;
    layoutFrame(F, a, FL);
    size_t off[13];
    for (int k = 0; k < 13; k++) off[k] = a.take(in[k].elem * M);
    const size_t inputBytes = a.off;
    const PassLayout PL = layoutPasses(ctx, a, M, N, true);
    const size_t oGrid = layoutGrid(a, N);
    const size_t oRaw = a.take(40 * (size_t)M);
    const size_t total = a.off;
    const size_t outBytes = 16 * (size_t)M + 40 * (size_t)M + 64;
    rc = ft_ensure_scratch(ctx, total, std::max(inputBytes, outBytes));
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    stageFrame(F, FL, pin);
    for (int k = 0; k < 13; k++) memcpy(pin + off[k], in[k].src, in[k].elem * M);
    hipStream_t st = ctx->stream;
    FT_HIP(hipMemcpyAsync(dev, pin, inputBytes, hipMemcpyHostToDevice, st));
    FtDevFrame DF = devFrame(F, FL, dev);
    rc = buildGrid(ctx, st, DF, (int *)(dev + oGrid));
    if (rc != FT_OK) return rc;
    for (int k = 0; k < 13; k++) *(const void **)in[k].dst = dev + off[k];
    int *rawBase = (int *)(dev + oRaw), *hRaw = (int *)(pin + 16 * (size_t)M + 64);
    int nm = 0, passes = 0;
    rc = runLocalSearch(ctx, DF, DP, passBufs(PL, dev, dObs), rawBase, nullptr, th, nn_ratio, pin, {hRaw, rawBase, 40 * (size_t)M},
                        P->observations, F->holder_obs, assign, &nm, &passes);
    if (rc != FT_OK) return rc;
    for (int k = 0; k < 10; k++)
        if (outs[k]) memcpy(outs[k], hRaw + (size_t)k * M, 4 * (size_t)M);
    if (n_matches) *n_matches = nm;
    ctx->addStat("search_local_points.total", tAll.ms());
    ctx->addStat("search_local_points.passes", passes);
    return FT_OK;
}

namespace {
int searchLastFrame(ft_context *ctx, ft_frame_view *Cur, const ft_last_points *L, const FtPose &pose, const FtPose *trl, float th,
                    int forward, int backward, int check_orientation, int *assign, int *n_matches, int *best_dist, int *best_idx,
                    int *best_dist_r, int *best_idx_r) {
    FT_REQUIRE(ctx && L && assign, "ft_search_last_frame: null argument");
    int rc = checkFrame(Cur);
    if (rc != FT_OK) return rc;
    const int M = L->N, N = Cur->N;
    rc = checkLastPoints(L, 0, -1, nullptr);
    if (rc != FT_OK) return rc;
    for (int i = 0; i < N; i++) assign[i] = -1;
    if (n_matches) *n_matches = 0;
    int *outs[4] = {best_dist, best_idx, best_dist_r, best_idx_r};
    if (M == 0 || N == 0) {
        for (int k = 0; k < 4; k++)
            if (outs[k])
                for (int i = 0; i < M; i++) outs[k][i] = (k % 2 == 0) ? 256 : -1;
        return FT_OK;
    }
    rc = checkLastPoints(L, Cur->nlevels, -1, nullptr);
    if (rc != FT_OK) return rc;
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    Arena a;
    FrameLayout FL;
    layoutFrame(Cur, a, FL);
    const LastLayout LL = layoutLast(a, M);
    const size_t inputBytes = a.off;
    const PassLayout PL = layoutPasses(ctx, a, M, N, true);
    const size_t oGrid = layoutGrid(a, N);
    const size_t oRaw = a.take(16 * (size_t)M);
    const size_t total = a.off;
    const size_t outBytes = 32 * (size_t)M + 64;
    rc = ft_ensure_scratch(ctx, total, std::max(inputBytes, outBytes));
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    stageFrame(Cur, FL, pin);
    stageLast(L, LL, pin);
    hipStream_t st = ctx->stream;
    FT_HIP(hipMemcpyAsync(dev, pin, inputBytes, hipMemcpyHostToDevice, st));
    FtDevFrame DF = devFrame(Cur, FL, dev);
    if (trl) setTrl(DF, *trl);
    rc = buildGrid(ctx, st, DF, (int *)(dev + oGrid));
    if (rc != FT_OK) return rc;
    int *rawBase = (int *)(dev + oRaw), *hRaw = (int *)(pin + 16 * (size_t)M + 64);
    auto curAngle = [&](int idx) -> float {
        return (Cur->Nleft == -1) ? Cur->keys[idx].angle
               : (idx < Cur->Nleft) ? Cur->keys[idx].angle
                                    : Cur->keys_right[idx - Cur->Nleft].angle;
    };
    int nm = 0, passes = 0;
    rc = runLastFrameSearch(ctx, DF, devLast(M, LL, dev), passBufs(PL, dev, (const int *)(dev + LL.obs)), rawBase, nullptr, pose, th, forward,
                            backward, pin, {hRaw, rawBase, 16 * (size_t)M}, L, check_orientation != 0, curAngle, Cur->holder_obs, assign, &nm,
                            &passes);
    if (rc != FT_OK) return rc;
    for (int k = 0; k < 4; k++)
        if (outs[k]) memcpy(outs[k], hRaw + (size_t)k * M, 4 * (size_t)M);
    if (n_matches) *n_matches = nm;
    ctx->addStat("search_last_frame.total", tAll.ms());
    ctx->addStat("search_last_frame.passes", passes);
    return FT_OK;
}
}  // namespace

int ft_search_last_frame(ft_context *ctx, ft_frame_view *Cur, const ft_last_points *L, const float *Tcw, float th,
                         int forward, int backward, int check_orientation, int *assign, int *n_matches,
                         int *best_dist, int *best_idx, int *best_dist_r, int *best_idx_r) {
    FT_REQUIRE(Tcw, "ft_search_last_frame: null pose");
    return searchLastFrame(ctx, Cur, L, poseOfMatrix(Tcw), nullptr, th, forward, backward, check_orientation, assign, n_matches,
                           best_dist, best_idx, best_dist_r, best_idx_r);
}

int ft_search_last_frame_se3(ft_context *ctx, ft_frame_view *Cur, const ft_last_points *L, const ft_se3 *Tcw, const ft_se3 *Trl,
                             float th, int forward, int backward, int check_orientation, int *assign, int *n_matches,
                             int *best_dist, int *best_idx, int *best_dist_r, int *best_idx_r) {
    FT_REQUIRE(Tcw && Cur, "ft_search_last_frame_se3: null argument");
    FtPose pose, trl;
    const FtPose *trlPtr = nullptr;
    const int rc = posesFromSe3(Tcw, Trl, Cur->Nleft != -1, "ft_search_last_frame_se3", pose, trl, &trlPtr);
    if (rc != FT_OK) return rc;
    return searchLastFrame(ctx, Cur, L, pose, trlPtr, th, forward, backward, check_orientation, assign, n_matches, best_dist, best_idx,
                           best_dist_r, best_idx_r);
}

int ft_features_in_area(ft_context *ctx, const ft_frame_view *F, int nq, const float *x, const float *y, const float *r,
                        const int *min_level, const int *max_level, const uint8_t *right, int *indices, int capacity,
                        int *counts) {
    FT_REQUIRE(ctx && counts && nq >= 0 && capacity >= 0, "ft_features_in_area: bad argument");
    FT_REQUIRE(nq == 0 || (x && y && r && min_level && max_level), "ft_features_in_area: null query arrays");
    FT_REQUIRE(capacity == 0 || indices, "ft_features_in_area: null index array");
    FT_REQUIRE(nq < (1 << 22), "ft_features_in_area: too many queries");
    int rc = checkFrame(F);
    if (rc != FT_OK) return rc;
    FT_REQUIRE(F->N < (1 << 20), "ft_features_in_area: frame too large for the hit keys");
    if (nq == 0) return FT_OK;
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    Arena a;
    FrameLayout FL;
    layoutFrame(F, a, FL);
    const size_t Q = (size_t)nq;
    const size_t oX = a.take(4 * Q), oY = a.take(4 * Q), oR = a.take(4 * Q), oMin = a.take(4 * Q), oMax = a.take(4 * Q),
                 oRight = a.take(Q);
    const size_t inputBytes = a.off;
    const size_t oCount = a.take(4 * Q), oOff = a.take(4 * Q);
    const size_t fixedBytes = a.off;
    rc = ft_ensure_scratch(ctx, fixedBytes, fixedBytes);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    hipStream_t st = ctx->stream;
    auto stageInputs = [&] {  // the frame and the queries into the pinned mirror
        stageFrame(F, FL, pin);
        memcpy(pin + oX, x, 4 * Q);
        memcpy(pin + oY, y, 4 * Q);
        memcpy(pin + oR, r, 4 * Q);
        memcpy(pin + oMin, min_level, 4 * Q);
        memcpy(pin + oMax, max_level, 4 * Q);
        if (right) memcpy(pin + oRight, right, Q);
    };
    auto launch = [&](const int *offsets, unsigned *keys) {
        return ft_launch_features_in_area(st, devFrame(F, FL, dev), nq, (const float *)(dev + oX), (const float *)(dev + oY),
                                          (const float *)(dev + oR), (const int *)(dev + oMin), (const int *)(dev + oMax),
                                          right ? dev + oRight : nullptr, offsets, keys, (int *)(dev + oCount));
    };
    CallEventTimer own;
    // phase 1 counts the hits of every query, phase 2 writes them at the query's offset (no capacity inside)
    stageInputs();
    CallScope C1{ctx, st, dev, pin, own.evt};
    C1.up(0, inputBytes);
    C1.launch(nullptr, [&] { return launch(nullptr, nullptr); });
    rc = C1.down(oCount, oCount + 4 * Q);
    if (rc != FT_OK) return rc;
    memcpy(counts, pin + oCount, 4 * Q);
    size_t totalHits = 0;
    for (int q = 0; q < nq; q++) totalHits += (size_t)counts[q];
    if (totalHits == 0) return FT_OK;
    FT_REQUIRE(totalHits < (1u << 30), "ft_features_in_area: too many hits");
    const size_t oKeys = a.take(4 * totalHits);
    // growing the scratch reallocates it (nothing is in flight: phase 1 has been waited for, and the counts are the caller's
    // by now): where the device side moved, the frame and the queries are staged and go up again
    const size_t devBytesBefore = ctx->scratchDevBytes;
    rc = ft_ensure_scratch(ctx, a.off, a.off);
    if (rc != FT_OK) return rc;
    pin = (uint8_t *)ctx->scratchPin, dev = (uint8_t *)ctx->scratchDev;
    CallScope C2{ctx, st, dev, pin, own.evt};
    if (ctx->scratchDevBytes != devBytesBefore) {
        stageInputs();
        C2.up(0, inputBytes);
    }
    int *hOff = (int *)(pin + oOff);
    for (int q = 0, at = 0; q < nq; at += counts[q++]) hOff[q] = at;
    C2.up(oOff, oOff + 4 * Q);
    C2.launch(nullptr, [&] { return launch((const int *)(dev + oOff), (unsigned *)(dev + oKeys)); });
    rc = C2.down(oKeys, oKeys + 4 * totalHits);
    if (rc != FT_OK) return rc;
    unsigned *hKeys = (unsigned *)(pin + oKeys);
    for (int q = 0; q < nq; q++) {
        unsigned *k = hKeys + hOff[q];
        std::sort(k, k + counts[q]);  // (cell column, cell row, index): the order of the nested loops of Frame.cc:718-744
        const int m = std::min(counts[q], capacity);
        for (int i = 0; i < m; i++) indices[(size_t)q * capacity + i] = (int)(k[i] & 0xfffffu);
    }
    return FT_OK;
}

int ft_is_in_frustum(ft_context *ctx, const ft_frame_view *F, const ft_frame_pose *pose, const ft_map_points *P,
                     float viewing_cos_limit, float log_scale_factor, const ft_frustum_result *out, int *n_to_match) {
    FT_REQUIRE(ctx && F && pose, "ft_is_in_frustum: null argument");
    FT_REQUIRE(F->nlevels >= 1 && F->nlevels <= FT_MAX_LEVELS, "ft_is_in_frustum: nlevels out of range");
    FT_REQUIRE(F->cam_model == 0 || F->cam_model == 1, "unknown camera model");
    int rc = checkMapPoints(P, false);
    if (rc != FT_OK) return rc;
    if (n_to_match) *n_to_match = 0;
    if (P->M == 0) return FT_OK;
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    Arena a;
    FrustumLayout L;
    size_t inputEnd = 0;
    layoutFrustum(P->M, P->skip != nullptr, a, L, &inputEnd);
    rc = ft_ensure_scratch(ctx, a.off, a.off);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    stageFrustum(P, L, pin);
    hipStream_t st = ctx->stream;
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, inputEnd);
    C.launch(nullptr, [&] {
        return ft_launch_frustum(st, devFrameConstants(F), frustumPose(F, pose), devMapPoints(P, L, dev), viewing_cos_limit, log_scale_factor,
                                 0, 0.f, devFrustumOut(L, dev));
    });
    rc = C.down(inputEnd, a.off);
    if (rc == FT_OK) unpackFrustum(P->M, L, inputEnd, pin + inputEnd, out, n_to_match);
    ctx->addStat("is_in_frustum.total", tAll.ms());
    return rc;
}

}  // extern "C"

// ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:2087-2208),
// the matcher Tracking::Relocalization calls behind PnP (src/Tracking.cc:3924, :3938).  The host enqueues: the keyframe's points
// and the pose up, k_reloc_project, k_reloc_candidates, k_reloc_resolve (kernels_reloc.hip), the results down - and waits once.
// Nothing of that sequence depends on what the frame or the keyframe hold.
#include "search_host.h"

namespace {

struct RelocLayout {
    size_t valid, pos, maxd, mind, desc, obs, angle, inputEnd;  // the keyframe's points
    size_t out, assign, bestDist, bestIdx, tail, outEnd;        // what comes back: assign | best_dist | best_idx | nmatches, status
    size_t proj, top, segCount, seg;
};
RelocLayout layoutReloc(Arena &a, int M, int N, bool wantBest) {
    RelocLayout L;
    const size_t m = (size_t)std::max(M, 1), n = (size_t)std::max(N, 1);
    L.valid = a.take(m);
    L.pos = a.take(12 * m);
    L.maxd = a.take(4 * m);
    L.mind = a.take(4 * m);
    L.desc = a.take(32 * m);
    L.obs = a.take(4 * m);
    L.angle = a.take(4 * m);
    L.inputEnd = a.off;
    L.out = a.off;
    L.assign = a.take(4 * n);
    L.bestDist = wantBest ? a.take(4 * m) : 0;
    L.bestIdx = wantBest ? a.take(4 * m) : 0;
    L.tail = a.take(64);
    L.outEnd = a.off;
    L.proj = a.take(sizeof(FtRelocProj) * m);
    L.top = a.take(8 * FT_RELOC_TOP * m);
    L.segCount = a.take(4 * m);
    L.seg = a.take(8 * (size_t)FT_RELOC_SEG * m);
    return L;
}
void stageReloc(const ft_keyframe_points *K, bool angles, const RelocLayout &L, uint8_t *pin) {
    const size_t M = (size_t)K->N;
    memcpy(pin + L.valid, K->valid, M);
    memcpy(pin + L.pos, K->world_pos, 12 * M);
    memcpy(pin + L.maxd, K->max_distance, 4 * M);
    memcpy(pin + L.mind, K->min_distance, 4 * M);
    memcpy(pin + L.desc, K->descriptors, 32 * M);
    memcpy(pin + L.obs, K->observations, 4 * M);
    if (angles) memcpy(pin + L.angle, K->angle, 4 * M);
}

// the arguments of both entry points that do not depend on the frame's form
int checkRelocArgs(const ft_keyframe_points *K, const ft_se3 *Tcw, float th, int orb_dist, int check_orientation, const char *what) {
    const std::string w(what);
    FT_REQUIRE(K && Tcw, w + ": null argument");
    FT_REQUIRE(K->N >= 0 && K->N < (1 << 22), w + ": keyframe point count out of range");
    FT_REQUIRE(K->N == 0 || (K->valid && K->world_pos && K->max_distance && K->min_distance && K->descriptors && K->observations),
               w + ": keyframe point arrays are null");
    FT_REQUIRE(K->N == 0 || !check_orientation || K->angle, w + ": the orientation check needs the keyframe's keypoint angles");
    FT_REQUIRE(th > 0.f, w + ": th must be positive");
    FT_REQUIRE(orb_dist >= 0 && orb_dist < 256, w + ": orb_dist outside [0, 255]");
    return FT_OK;
}
bool anyValid(const ft_keyframe_points *K) {
    for (int i = 0; i < K->N; i++)
        if (K->valid[i]) return true;
    return false;
}
int checkRelocCaps(int nLeft, int M) {
    if (ft_reloc_lds_bytes(nLeft, M) > FT_INIT_MAX_LDS) {
        ft_set_error("SearchByProjection(Frame, KeyFrame): too many keyframe points / keypoints (the tables of the resolution hold 4 bytes "
                     "per point and a bit per keypoint in 150 KB)");
        return FT_ERR_CAPACITY;
    }
    return FT_OK;
}

// S: F (with its grid), holder and the call's parameters are set; C: the arena of layout L and its pinned mirror, the points are
// staged in pin.  Returns with assign / best / tail in pin; FT_ERR_CAPACITY (nothing written, the device's holder_obs included)
// when a point's candidates exceed its segment.
int runRelocSearch(CallScope &C, FtRelocSearch S, const RelocLayout &L, bool wantBest) {
    uint8_t *dev = C.dev;
    C.up(L.valid, L.inputEnd);
    C.zero(L.tail, L.tail + 64);
    S.valid = dev + L.valid;
    S.worldPos = (const float *)(dev + L.pos);
    S.maxDist = (const float *)(dev + L.maxd);
    S.minDist = (const float *)(dev + L.mind);
    S.desc = dev + L.desc;
    S.obs = (const int *)(dev + L.obs);
    S.angle = (const float *)(dev + L.angle);
    S.proj = (FtRelocProj *)(dev + L.proj);
    S.top = (unsigned long long *)(dev + L.top);
    S.seg = (unsigned long long *)(dev + L.seg);
    S.segCount = (int *)(dev + L.segCount);
    S.assign = (int *)(dev + L.assign);
    S.bestDist = wantBest ? (int *)(dev + L.bestDist) : nullptr;
    S.bestIdx = wantBest ? (int *)(dev + L.bestIdx) : nullptr;
    S.nMatches = (int *)(dev + L.tail);
    S.status = (int *)(dev + L.tail) + 4;
    C.launch("kernel.reloc_project", [&] { return ft_launch_reloc_project(C.st, S); });
    C.launch("kernel.reloc_candidates", [&] { return ft_launch_reloc_candidates(C.st, S); });
    C.launch("kernel.reloc_resolve", [&] { return ft_launch_reloc_resolve(C.st, S); });
    const int rc = C.down(L.out, L.outEnd);
    if (rc != FT_OK) return rc;
    if (((const int *)(C.pin + L.tail))[4] != 0) {
        ft_set_error("SearchByProjection(Frame, KeyFrame): a point's window holds more than 256 free keypoints of its level band");
        return FT_ERR_CAPACITY;
    }
    return FT_OK;
}

// holder_obs as the call leaves it: a surviving write carries the point's Observations() (an entry the histogram removed was
// free on entry and is free again)
void applyAssign(const int *assign, int N, const int *observations, int *holder) {
    for (int k = 0; k < N; k++)
        if (assign[k] >= 0) holder[k] = observations[assign[k]];
}
}  // namespace

extern "C" {

int ft_search_keyframe_projection(ft_context *ctx, ft_frame_view *Cur, const ft_keyframe_points *K, const ft_se3 *Tcw, float log_scale_factor,
                                  float th, int orb_dist, int check_orientation, int *assign, int *n_matches, int *best_dist, int *best_idx) {
    FT_REQUIRE(ctx, "ft_search_keyframe_projection: null context");
    int rc = checkRelocArgs(K, Tcw, th, orb_dist, check_orientation, "ft_search_keyframe_projection");
    if (rc != FT_OK) return rc;
    rc = checkFrame(Cur);
    if (rc != FT_OK) return rc;
    const int M = K->N, N = Cur->N, nLeft = Cur->Nleft == -1 ? N : Cur->Nleft;
    FT_REQUIRE(N == 0 || assign, "ft_search_keyframe_projection: null assign");
    FtPose pose;
    rc = poseOfSe3(Tcw, pose);
    if (rc != FT_OK) return rc;
    auto defaults = [&]() {
        for (int i = 0; i < N; i++) assign[i] = -1;
        if (n_matches) *n_matches = 0;
        for (int i = 0; i < M; i++) {
            if (best_dist) best_dist[i] = 256;
            if (best_idx) best_idx[i] = -1;
        }
    };
    if (M == 0 || nLeft == 0 || !anyValid(K)) {
        defaults();
        return FT_OK;
    }
    rc = checkRelocCaps(nLeft, M);
    if (rc != FT_OK) return rc;
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    const bool wantBest = best_dist || best_idx;
    Arena a;
    FrameLayout FL;
    layoutFrame(Cur, a, FL);
    const size_t frameBytes = a.off;
    const RelocLayout L = layoutReloc(a, M, N, wantBest);
    const size_t oGrid = layoutGrid(a, N);
    rc = ft_ensure_scratch(ctx, a.off, L.outEnd);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    stageFrame(Cur, FL, pin);
    stageReloc(K, check_orientation != 0, L, pin);
    CallEventTimer own;
    CallScope C{ctx, ctx->stream, dev, pin, own.evt};
    C.up(0, frameBytes);
    FtRelocSearch S;
    memset(&S, 0, sizeof S);
    S.F = devFrame(Cur, FL, dev);
    // the grid of the frame, whatever option search_grid says for the other projection searches: this one walks nothing else
    C.launch(nullptr, [&] { return launchGrid(C.st, S.F, (int *)(dev + oGrid)); });
    S.N = M;
    S.Tcw = pose;
    S.logScaleFactor = log_scale_factor;
    S.th = th;
    S.orbDist = orb_dist;
    S.checkOrientation = check_orientation != 0;
    S.holder = (int *)(dev + FL.holder);
    rc = runRelocSearch(C, S, L, wantBest);
    if (rc != FT_OK) return rc;
    memcpy(assign, pin + L.assign, 4 * (size_t)N);
    if (best_dist) memcpy(best_dist, pin + L.bestDist, 4 * (size_t)M);
    if (best_idx) memcpy(best_idx, pin + L.bestIdx, 4 * (size_t)M);
    if (n_matches) *n_matches = *(const int *)(pin + L.tail);
    applyAssign(assign, N, K->observations, Cur->holder_obs);
    ctx->addStat("search_keyframe_projection.total", tAll.ms());
    ctx->addStat("search_keyframe_projection.launches", C.launches);
    return FT_OK;
}

int ft_tracked_frame_search_keyframe_projection(ft_tracked_frame *tf, const ft_keyframe_points *K, const ft_se3 *Tcw, float log_scale_factor,
                                                float th, int orb_dist, int check_orientation, int *assign, int *n_matches) {
    FT_REQUIRE(tf && tf->loaded, "ft_tracked_frame_search_keyframe_projection: null tracked frame / no frame loaded");
    int rc = checkRelocArgs(K, Tcw, th, orb_dist, check_orientation, "ft_tracked_frame_search_keyframe_projection");
    if (rc != FT_OK) return rc;
    ft_context *ctx = tf->ctx;
    const int M = K->N, N = tf->DF.N, nLeft = tf->DF.Nleft == -1 ? N : tf->DF.Nleft;
    FT_REQUIRE(N == 0 || assign, "ft_tracked_frame_search_keyframe_projection: null assign");
    FtPose pose;
    rc = poseOfSe3(Tcw, pose);
    if (rc != FT_OK) return rc;
    if (M == 0 || nLeft == 0 || !anyValid(K)) {
        for (int i = 0; i < N; i++) assign[i] = -1;
        if (n_matches) *n_matches = 0;
        return FT_OK;
    }
    rc = checkRelocCaps(nLeft, M);
    if (rc != FT_OK) return rc;
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    Arena a;
    const RelocLayout L = layoutReloc(a, M, N, false);
    rc = ensureInitArena(tf, a.off, L.outEnd);
    if (rc != FT_OK) return rc;
    CallScope C{ctx, ctx->stream, tf->d_init, tf->h_init, tf->evt};
    stageReloc(K, check_orientation != 0, L, C.pin);
    FtRelocSearch S;
    memset(&S, 0, sizeof S);
    S.F = tf->DF;
    // option search_grid = 0 when the frame was loaded: the grid for this call
    if (!S.F.gridStart[0]) C.launch(nullptr, [&] { return launchGrid(C.st, S.F, tf->d_grid); });
    S.N = M;
    S.Tcw = pose;
    S.logScaleFactor = log_scale_factor;
    S.th = th;
    S.orbDist = orb_dist;
    S.checkOrientation = check_orientation != 0;
    S.holder = tf->d_holder;  // the resident occupancy, updated where it is: the next search on this frame sees it
    rc = runRelocSearch(C, S, L, false);
    if (rc != FT_OK) return rc;
    memcpy(assign, C.pin + L.assign, 4 * (size_t)N);
    if (n_matches) *n_matches = *(const int *)(C.pin + L.tail);
    applyAssign(assign, N, K->observations, tf->holder.data());
    ctx->addStat("tracked.search_keyframe_projection.total", tAll.ms());
    ctx->addStat("tracked.search_keyframe_projection.launches", C.launches);
    return FT_OK;
}

}  // extern "C"

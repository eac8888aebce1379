// ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) and Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1247-1437,
// :1439-1554), the searches LocalMapping::SearchInNeighbors runs for every target keyframe and camera (src/LocalMapping.cc:772-803)
// and LoopClosing::SearchAndFuse for every keyframe of the corrected window (src/LoopClosing.cc:2133, :2178): here one list of map
// points against every target of a call.  The host packs the points, every target's searched camera and the target records into
// one pinned block and enqueues: the block up, k_fuse_grid, k_fuse_search (kernels_fuse.hip), the results down - and waits once.
// Nothing of that sequence depends on the number of targets or points or on what the keyframes hold.
#include <vector>

#include "search_host.h"

namespace {

struct FuseLayout {
    size_t keys, desc, uright, valid;  // staged
    size_t grid;                       // device only
};

int checkFuseTarget(const ft_fuse_target *t, int k, FuseSide &s) {
    const std::string w = "ft_fuse_search: target " + std::to_string(k) + ": ";
    const int rc = checkKeyframeSide(t->kf, t->right != 0, w, s);
    if (rc != FT_OK) return rc;
    FT_REQUIRE(!t->check_reprojection || t->inv_level_sigma2, w + "the reprojection test needs inv_level_sigma2");
    FT_REQUIRE(t->th > 0.f, w + "th must be positive");
    return FT_OK;
}

}  // namespace

extern "C" {

int ft_fuse_search(ft_context *ctx, const ft_fuse_points *P, int n_targets, const ft_fuse_target *targets, int *best_idx, int *best_dist,
                   uint8_t *stage, int *n_found) {
    FT_REQUIRE(ctx && P, "ft_fuse_search: null argument");
    FT_REQUIRE(n_targets >= 0 && n_targets < (1 << 16), "ft_fuse_search: n_targets out of range");
    int rc = checkPoints(*P, "ft_fuse_search: ");
    if (rc != FT_OK) return rc;
    const int M = P->M;
    FT_REQUIRE(n_targets == 0 || (targets && n_found), "ft_fuse_search: null targets or n_found");
    FT_REQUIRE(n_targets == 0 || M == 0 || (best_idx && best_dist), "ft_fuse_search: null best_idx or best_dist");
    std::vector<FuseSide> sides((size_t)n_targets);
    std::vector<FtPose> poses((size_t)n_targets);
    int maxLevels = 1;
    for (int k = 0; k < n_targets; k++) {
        rc = checkFuseTarget(targets + k, k, sides[k]);
        if (rc == FT_OK) rc = poseOfSe3(&targets[k].Tcw, poses[k]);
        if (rc != FT_OK) return rc;
        maxLevels = std::max(maxLevels, targets[k].kf->nlevels);
    }
    for (int k = 0; k < n_targets; k++) n_found[k] = 0;
    if (n_targets == 0 || M == 0) return FT_OK;
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    // the arena: points | every target's camera (keypoints, descriptors, mvuRight, valid) | target records | n_found || best_idx |
    // best_dist | stage ||| the grids (device only).  One copy up: [0, inputEnd); one copy down: [oFound, outEnd).
    const size_t m = (size_t)M, rows = m * (size_t)n_targets;
    Arena a;
    const PointsLayout PL = layoutPoints(a, m);
    std::vector<FuseLayout> L((size_t)n_targets);
    for (int k = 0; k < n_targets; k++) {
        const size_t n = (size_t)std::max(sides[k].n, 1);
        L[k].keys = a.take(sizeof(ft_keypoint) * n);
        L[k].desc = a.take(32 * n);
        L[k].uright = sides[k].uright ? a.take(4 * n) : 0;
        L[k].valid = targets[k].valid ? a.take(m) : 0;
    }
    const size_t oTargets = a.take(sizeof(FtFuseTarget) * (size_t)n_targets);
    const size_t oFound = a.take(4 * (size_t)n_targets);
    const size_t inputEnd = a.off;
    const size_t oBestIdx = a.take(4 * rows), oBestDist = a.take(4 * rows);
    const size_t oStage = stage ? a.take(rows) : 0;
    const size_t outEnd = a.off;
    for (int k = 0; k < n_targets; k++) L[k].grid = a.take(sideGridBytes(targets[k].kf->nlevels, sides[k].n));
    rc = ft_ensure_scratch(ctx, a.off, outEnd);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    stagePoints(P, PL, pin);
    FtFuseTarget *recs = (FtFuseTarget *)(pin + oTargets);
    memset(recs, 0, sizeof(FtFuseTarget) * (size_t)n_targets);
    for (int k = 0; k < n_targets; k++) {
        const ft_fuse_target &t = targets[k];
        const FuseSide &s = sides[k];
        const size_t n = (size_t)s.n;
        if (n) {
            memcpy(pin + L[k].keys, s.keys, sizeof(ft_keypoint) * n);
            memcpy(pin + L[k].desc, s.desc, 32 * n);
            if (s.uright) memcpy(pin + L[k].uright, s.uright, 4 * n);
        }
        if (t.valid) memcpy(pin + L[k].valid, t.valid, m);
        FtFuseTarget &R = recs[k];
        R.F = devFrameConstants(t.kf);
        R.F.N = s.n;
        R.F.Nleft = -1;
        if (t.right) memcpy(R.F.cam, t.cam2, sizeof R.F.cam);
        R.F.keys = (const ft_keypoint *)(dev + L[k].keys);
        R.F.desc = dev + L[k].desc;
        R.F.uright = s.uright ? (const float *)(dev + L[k].uright) : nullptr;
        pointSideGrid(R.F, dev + L[k].grid, t.kf->nlevels, s.n);
        R.Tcw = poses[k];
        memcpy(R.Ow, t.Ow, sizeof R.Ow);
        R.logScaleFactor = t.log_scale_factor;
        R.th = t.th;
        if (t.check_reprojection) memcpy(R.invSigma2, t.inv_level_sigma2, 4 * (size_t)t.kf->nlevels);
        R.checkReproj = t.check_reprojection != 0;
        R.idxOffset = s.idxOffset;
        R.valid = t.valid ? dev + L[k].valid : nullptr;
        R.bestIdx = (int *)(dev + oBestIdx) + m * (size_t)k;
        R.bestDist = (int *)(dev + oBestDist) + m * (size_t)k;
        R.stage = stage ? dev + oStage + m * (size_t)k : nullptr;
        R.nFound = (int *)(dev + oFound) + k;
    }
    memset(pin + oFound, 0, 4 * (size_t)n_targets);
    const FtFusePoints DP = devPoints(M, PL, dev);
    const FtFuseTarget *dTargets = (const FtFuseTarget *)(dev + oTargets);
    hipStream_t st = ctx->stream;
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, inputEnd);  // one copy: the block is contiguous
    C.launch("kernel.fuse_grid", [&] { return ft_launch_fuse_grid(st, dev, dTargets, n_targets, maxLevels); });
    C.launch("kernel.fuse_search", [&] { return ft_launch_fuse_search(st, dev, dTargets, n_targets, DP); });
    rc = C.down(oFound, outEnd);
    if (rc != FT_OK) return rc;
    memcpy(n_found, pin + oFound, 4 * (size_t)n_targets);
    memcpy(best_idx, pin + oBestIdx, 4 * rows);
    memcpy(best_dist, pin + oBestDist, 4 * rows);
    if (stage) memcpy(stage, pin + oStage, rows);
    ctx->addStat("fuse.total", tAll.ms());
    ctx->addStat("fuse.launches", C.launches);
    return FT_OK;
}

}  // extern "C"

// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) and its overload with vpPointsKFs / vpMatchedKF
// (src/ORBmatcher.cc:526-631, :633-745), the matchers of LoopClosing::FindMatchesByProjection (src/LoopClosing.cc:755, :777, :964):
// here every search a caller has against ONE keyframe in one call.  The host packs the keyframe's left camera, every job's points,
// vpMatched and the job records into one pinned block and enqueues: the block up, k_sim3_grid, k_sim3_candidates, k_sim3_resolve
// (kernels_sim3.hip), the results down - and waits once.  Nothing of that sequence depends on the number of jobs or on what they hold.
#include <vector>

#include "search_host.h"

namespace {

struct Sim3Layout {
    PointsLayout pts;                          // staged
    size_t valid;
    size_t matched;                            // staged and returned
    size_t nMatches, pointKeypoint, stage;     // returned
    size_t proj, top, count, walk;             // device only
};

// `bestDist<=TH_LOW*ratioHamming` (:622): an int converted to float against the float product of the int 50 and the float ratio
int sim3Threshold(float ratio, int &thr) {
    const float prod = (float)FT_TH_LOW * ratio;
    if (!(prod >= 0.0f && prod < 256.0f)) {
        ft_set_error("ft_search_keyframe_sim3: 50 * ratio_hamming must lie in [0, 256)");
        return FT_ERR_INVALID;
    }
    thr = (int)prod;  // the largest d with (float)d <= prod: every d of 0 .. 255 is a float
    return FT_OK;
}

int checkSim3Job(const ft_sim3_job &j, int k, int N, FtPose &pose, int &thr) {
    const std::string w = "ft_search_keyframe_sim3: job " + std::to_string(k) + ": ";
    int rc = checkPoints(j.points, w);
    if (rc != FT_OK) return rc;
    FT_REQUIRE(N == 0 || j.matched, w + "null matched");
    FT_REQUIRE(j.th > 0, w + "th must be positive");
    rc = sim3Threshold(j.ratio_hamming, thr);
    if (rc != FT_OK) return rc;
    return poseOfSe3(&j.Tcw, pose);
}

}  // namespace

extern "C" {

int ft_search_keyframe_sim3(ft_context *ctx, const ft_frame_view *kf, int n_jobs, ft_sim3_job *jobs) {
    FT_REQUIRE(ctx, "ft_search_keyframe_sim3: null context");
    FT_REQUIRE(n_jobs >= 0 && n_jobs < (1 << 16), "ft_search_keyframe_sim3: n_jobs out of range");
    FT_REQUIRE(n_jobs == 0 || jobs, "ft_search_keyframe_sim3: null jobs");
    FuseSide side;  // the left camera
    int rc = checkKeyframeSide(kf, false, "ft_search_keyframe_sim3: ", side);
    if (rc != FT_OK) return rc;
    const int nLeft = side.n;
    std::vector<FtPose> poses((size_t)n_jobs);
    std::vector<int> thrs((size_t)n_jobs);
    int maxM = 0;
    for (int k = 0; k < n_jobs; k++) {
        rc = checkSim3Job(jobs[k], k, kf->N, poses[k], thrs[k]);
        if (rc != FT_OK) return rc;
        maxM = std::max(maxM, jobs[k].points.M);
    }
    if (ft_sim3_lds_bytes(nLeft) > FT_INIT_MAX_LDS) {
        ft_set_error("ft_search_keyframe_sim3: more than 1 228 800 left keypoints (the resolution keeps a taken bit per keypoint in 150 KB)");
        return FT_ERR_CAPACITY;
    }
    if (n_jobs == 0 || maxM == 0 || nLeft == 0) {
        for (int k = 0; k < n_jobs; k++) {
            ft_sim3_job &j = jobs[k];
            j.n_matches = 0;
            for (int i = 0; i < j.points.M; i++) {
                if (j.point_keypoint) j.point_keypoint[i] = -1;
                if (j.stage) j.stage[i] = FT_FUSE_EMPTY;
            }
        }
        return FT_OK;
    }
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    // the arena: keypoints, descriptors | every job's points | job records | every job's matched || n_matches, point_keypoint,
    // stage ||| candidate records, walk lists, the grid (device only).  One copy up: [0, inputEnd); one copy down: [outBegin, outEnd).
    const size_t n = (size_t)nLeft;
    Arena a;
    const size_t oKeys = a.take(sizeof(ft_keypoint) * n), oKfDesc = a.take(32 * n);
    std::vector<Sim3Layout> L((size_t)n_jobs);
    for (int k = 0; k < n_jobs; k++) {
        const size_t m = (size_t)jobs[k].points.M;
        L[k].pts = layoutPoints(a, m);
        L[k].valid = jobs[k].valid ? a.take(m) : 0;
    }
    const size_t oJobs = a.take(sizeof(FtSim3Job) * (size_t)n_jobs);
    const size_t outBegin = a.off;
    for (int k = 0; k < n_jobs; k++) L[k].matched = a.take(4 * n);
    const size_t inputEnd = a.off;
    for (int k = 0; k < n_jobs; k++) {
        const size_t m = (size_t)jobs[k].points.M;
        L[k].nMatches = a.take(4);
        L[k].pointKeypoint = a.take(4 * m);
        L[k].stage = a.take(m);
    }
    const size_t outEnd = a.off;
    for (int k = 0; k < n_jobs; k++) {
        const size_t m = (size_t)jobs[k].points.M;
        L[k].proj = a.take(sizeof(FtSim3Proj) * m);
        L[k].top = a.take(8 * FT_SIM3_TOP * m);
        L[k].count = a.take(4 * m);
        L[k].walk = a.take(4 * m);
    }
    const size_t oGrid = a.take(sideGridBytes(kf->nlevels, nLeft));
    rc = ft_ensure_scratch(ctx, a.off, outEnd);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    memcpy(pin + oKeys, kf->keys, sizeof(ft_keypoint) * n);
    memcpy(pin + oKfDesc, kf->descriptors, 32 * n);
    FtSim3Job *recs = (FtSim3Job *)(pin + oJobs);
    memset(recs, 0, sizeof(FtSim3Job) * (size_t)n_jobs);
    for (int k = 0; k < n_jobs; k++) {
        const ft_sim3_job &j = jobs[k];
        stagePoints(&j.points, L[k].pts, pin);
        if (j.valid && j.points.M) memcpy(pin + L[k].valid, j.valid, (size_t)j.points.M);
        memcpy(pin + L[k].matched, j.matched, 4 * n);
        FtSim3Job &R = recs[k];
        R.P = devPoints(j.points.M, L[k].pts, dev);
        R.valid = j.valid ? dev + L[k].valid : nullptr;
        R.Tcw = poses[k];
        memcpy(R.Ow, j.Ow, sizeof R.Ow);
        R.logScaleFactor = j.log_scale_factor;
        R.th = (float)j.th;
        R.thr = thrs[k];
        R.handPinhole = j.hand_pinhole != 0;
        R.wantStage = j.stage != nullptr;
        R.matched = (int *)(dev + L[k].matched);
        R.pointKeypoint = (int *)(dev + L[k].pointKeypoint);
        R.stage = dev + L[k].stage;
        R.nMatches = (int *)(dev + L[k].nMatches);
        R.proj = (FtSim3Proj *)(dev + L[k].proj);
        R.top = (unsigned long long *)(dev + L[k].top);
        R.count = (int *)(dev + L[k].count);
        R.walk = (int *)(dev + L[k].walk);
    }
    // the left camera as a one-camera frame with its grid
    FtDevFrame F = devFrameConstants(kf);
    F.N = nLeft;
    F.Nleft = -1;
    F.keys = (const ft_keypoint *)(dev + oKeys);
    F.desc = dev + oKfDesc;
    pointSideGrid(F, dev + oGrid, kf->nlevels, nLeft);
    const FtSim3Job *dJobs = (const FtSim3Job *)(dev + oJobs);
    hipStream_t st = ctx->stream;
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, inputEnd);  // one copy: the block is contiguous
    C.launch("kernel.sim3_grid", [&] { return ft_launch_sim3_grid(st, F); });
    C.launch("kernel.sim3_candidates", [&] { return ft_launch_sim3_candidates(st, F, dev, dJobs, n_jobs, maxM); });
    C.launch("kernel.sim3_resolve", [&] { return ft_launch_sim3_resolve(st, F, dev, dJobs, n_jobs); });
    rc = C.down(outBegin, outEnd);
    if (rc != FT_OK) return rc;
    for (int k = 0; k < n_jobs; k++) {
        ft_sim3_job &j = jobs[k];
        const size_t m = (size_t)j.points.M;
        memcpy(j.matched, pin + L[k].matched, 4 * n);
        j.n_matches = *(const int *)(pin + L[k].nMatches);
        if (j.point_keypoint && m) memcpy(j.point_keypoint, pin + L[k].pointKeypoint, 4 * m);
        if (j.stage && m) memcpy(j.stage, pin + L[k].stage, m);
    }
    ctx->addStat("sim3.total", tAll.ms());
    ctx->addStat("sim3.launches", C.launches);
    return FT_OK;
}

}  // extern "C"

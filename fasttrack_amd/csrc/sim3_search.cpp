// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) and its overload with vpPointsKFs / vpMatchedKF
// (src/ORBmatcher.cc:526-631, :633-745), the matchers of LoopClosing::FindMatchesByProjection (src/LoopClosing.cc:755, :777, :964):
// here every search a caller has against ONE keyframe in one call.  The host packs the keyframe's left camera, every job's points,
// vpMatched and the job records into one pinned block and enqueues: the block up, k_sim3_grid, k_sim3_candidates, k_sim3_resolve
// (kernels_sim3.hip), the results down - and waits once.  Nothing of that sequence depends on the number of jobs or on what they hold.
#include <vector>

#include "search_host.h"

namespace {

struct Sim3Layout {
    size_t pos, nrm, maxd, mind, desc, valid;  // staged
    size_t matched;                            // staged and returned
    size_t nMatches, pointKeypoint, stage;     // returned
    size_t proj, top, count, walk;             // device only
};

int checkSim3Keyframe(const ft_frame_view *F, int &nLeft) {
    const std::string w = "ft_search_keyframe_sim3: ";
    FT_REQUIRE(F, w + "null keyframe view");
    FT_REQUIRE(F->N >= 0 && F->N < (1 << 24), w + "keypoint count out of range");
    FT_REQUIRE(F->Nleft == -1 || (F->Nleft >= 0 && F->Nleft <= F->N), w + "Nleft out of range");
    FT_REQUIRE(F->cam_model == 0 || F->cam_model == 1, w + "unknown camera model");
    FT_REQUIRE(F->scale_factors && F->nlevels >= 1 && F->nlevels <= FT_MAX_LEVELS, w + "scale factors missing");
    nLeft = F->Nleft == -1 ? F->N : F->Nleft;
    FT_REQUIRE(nLeft == 0 || (F->keys && F->descriptors), w + "keypoints or descriptors are null");
    // the search reads a keypoint's octave back from four bits of its key (make_key, search_dev.h)
    for (int i = 0; i < nLeft; i++) FT_REQUIRE(F->keys[i].octave >= 0 && F->keys[i].octave < F->nlevels, w + "keypoint octave outside [0, nlevels)");
    return FT_OK;
}

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
    const ft_fuse_points &P = j.points;
    FT_REQUIRE(P.M >= 0 && P.M < (1 << 22), w + "map point count out of range");
    FT_REQUIRE(P.M == 0 || (P.world_pos && P.normal && P.max_distance && P.min_distance && P.descriptors), w + "map point arrays are null");
    FT_REQUIRE(N == 0 || j.matched, w + "null matched");
    FT_REQUIRE(j.th > 0, w + "th must be positive");
    int rc = sim3Threshold(j.ratio_hamming, thr);
    if (rc != FT_OK) return rc;
    return poseOfSe3(&j.Tcw, pose);
}

size_t sim3StartBytes(int nlevels) { return (sizeof(int) * (size_t)nlevels * (FT_GRID_CELLS + 1) + 63) & ~(size_t)63; }

}  // namespace

extern "C" {

int ft_search_keyframe_sim3(ft_context *ctx, const ft_frame_view *kf, int n_jobs, ft_sim3_job *jobs) {
    FT_REQUIRE(ctx, "ft_search_keyframe_sim3: null context");
    FT_REQUIRE(n_jobs >= 0 && n_jobs < (1 << 16), "ft_search_keyframe_sim3: n_jobs out of range");
    FT_REQUIRE(n_jobs == 0 || jobs, "ft_search_keyframe_sim3: null jobs");
    int nLeft = 0;
    int rc = checkSim3Keyframe(kf, nLeft);
    if (rc != FT_OK) return rc;
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
        L[k].pos = a.take(12 * m);
        L[k].nrm = a.take(12 * m);
        L[k].maxd = a.take(4 * m);
        L[k].mind = a.take(4 * m);
        L[k].desc = a.take(32 * m);
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
    const size_t oGrid = a.take(sim3StartBytes(kf->nlevels) + 48 * n);
    rc = ft_ensure_scratch(ctx, a.off, outEnd);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    memcpy(pin + oKeys, kf->keys, sizeof(ft_keypoint) * n);
    memcpy(pin + oKfDesc, kf->descriptors, 32 * n);
    FtSim3Job *recs = (FtSim3Job *)(pin + oJobs);
    memset(recs, 0, sizeof(FtSim3Job) * (size_t)n_jobs);
    for (int k = 0; k < n_jobs; k++) {
        const ft_sim3_job &j = jobs[k];
        const ft_fuse_points &P = j.points;
        const size_t m = (size_t)P.M;
        if (m) {
            memcpy(pin + L[k].pos, P.world_pos, 12 * m);
            memcpy(pin + L[k].nrm, P.normal, 12 * m);
            memcpy(pin + L[k].maxd, P.max_distance, 4 * m);
            memcpy(pin + L[k].mind, P.min_distance, 4 * m);
            memcpy(pin + L[k].desc, P.descriptors, 32 * m);
            if (j.valid) memcpy(pin + L[k].valid, j.valid, m);
        }
        memcpy(pin + L[k].matched, j.matched, 4 * n);
        FtSim3Job &R = recs[k];
        R.M = P.M;
        R.worldPos = (const float *)(dev + L[k].pos);
        R.normal = (const float *)(dev + L[k].nrm);
        R.maxDist = (const float *)(dev + L[k].maxd);
        R.minDist = (const float *)(dev + L[k].mind);
        R.desc = dev + L[k].desc;
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
    uint8_t *grid = dev + oGrid;
    float4 *rec = (float4 *)(grid + sim3StartBytes(kf->nlevels));
    F.gridStart[0] = (const int *)grid;
    F.gridRec[0] = rec;
    F.gridDesc[0] = (const uint8_t *)(rec + n);
    const FtSim3Job *dJobs = (const FtSim3Job *)(dev + oJobs);
    hipStream_t st = ctx->stream;
    FT_HIP(hipMemcpyAsync(dev, pin, inputEnd, hipMemcpyHostToDevice, st));  // one copy: the block is contiguous
    const bool tm = ctx->kernelTiming;
    FtEventTimer evt;
    evt.begin(tm, "kernel.sim3_grid", st);
    rc = ft_launch_sim3_grid(st, F);
    evt.end(tm, st);
    if (rc == FT_OK) {
        evt.begin(tm, "kernel.sim3_candidates", st);
        rc = ft_launch_sim3_candidates(st, F, dev, dJobs, n_jobs, maxM);
        evt.end(tm, st);
    }
    if (rc == FT_OK) {
        evt.begin(tm, "kernel.sim3_resolve", st);
        rc = ft_launch_sim3_resolve(st, F, dev, dJobs, n_jobs);
        evt.end(tm, st);
    }
    if (rc != FT_OK) {
        hipStreamSynchronize(st);
        evt.destroy();
        return rc;
    }
    hipError_t e = hipMemcpyAsync(pin + outBegin, dev + outBegin, outEnd - outBegin, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        evt.destroy();
        FT_HIP(e);
    }
    evt.resolve(ctx);
    evt.destroy();
    for (int k = 0; k < n_jobs; k++) {
        ft_sim3_job &j = jobs[k];
        const size_t m = (size_t)j.points.M;
        memcpy(j.matched, pin + L[k].matched, 4 * n);
        j.n_matches = *(const int *)(pin + L[k].nMatches);
        if (j.point_keypoint && m) memcpy(j.point_keypoint, pin + L[k].pointKeypoint, 4 * m);
        if (j.stage && m) memcpy(j.stage, pin + L[k].stage, m);
    }
    ctx->addStat("sim3.total", tAll.ms());
    ctx->addStat("sim3.launches", 3);
    return FT_OK;
}

}  // extern "C"

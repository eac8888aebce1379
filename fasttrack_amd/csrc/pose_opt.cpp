// Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:814-1114) for every frame of a call: ft_pose_optimization.  The host checks
// the frames and gathers each frame's correspondences in keypoint order into 32-byte edge records (:858-993: which edge a keypoint
// gets, its observation, its information, its map point) - straight from the caller's arrays into the pinned mirror of the arena,
// so an array is read where it lies, pinned or pageable, and no array is copied as a whole.  Then one block up (jobs and edges),
// ONE launch of k_pose_opt (kernels_pose_opt.hip: a workgroup per frame runs the four rounds), the results down, one wait.  A frame
// with fewer than three correspondences is answered here (:996) and has no job.  Nothing of the sequence depends on the number of frames.
#include "search_host.h"

namespace {

const char *const FN = "ft_pose_optimization";

int checkPoseOptFrame(const std::string &w, const ft_pose_opt_frame *F, uint8_t *outlier, int *nEdges) {
    FT_REQUIRE(F->N >= 0 && F->N < (1 << 24), w + "N out of range");
    FT_REQUIRE(F->Nleft == -1 || (F->Nleft >= 0 && F->Nleft <= F->N), w + "Nleft out of range");
    FT_REQUIRE(F->nlevels >= 1 && F->nlevels <= FT_MAX_LEVELS && F->inv_level_sigma2, w + "inv_level_sigma2 missing or nlevels out of range");
    FT_REQUIRE(F->cam_model == 0 || F->cam_model == 1, w + "unknown camera model");
    const int nL = F->Nleft == -1 ? F->N : F->Nleft, nR = F->N - nL;
    FT_REQUIRE(F->N == 0 || (F->has_point && F->world_pos && outlier), w + "has_point, world_pos or outlier is null");
    FT_REQUIRE(nL == 0 || F->keys, w + "keys is null");
    FT_REQUIRE(nR == 0 || F->keys_right, w + "keys_right is null");
    FtPose p;
    int rc = poseOfSe3(&F->Tcw, p);
    if (rc == FT_OK && F->Nleft != -1) rc = poseOfSe3(&F->Trl, p);
    if (rc != FT_OK) {
        ft_set_error(w + "Tcw.q / Trl.q is not a unit quaternion (x, y, z, w)");
        return rc;
    }
    int n = 0;
    for (int i = 0; i < F->N; i++) {
        if (!F->has_point[i]) continue;
        const int oct = i < nL ? F->keys[i].octave : F->keys_right[i - nL].octave;
        FT_REQUIRE(oct >= 0 && oct < F->nlevels, w + "the octave of a correspondence is outside [0, nlevels)");
        n++;
    }
    *nEdges = n;
    return FT_OK;
}

// :858-993 for the correspondences of F, in keypoint order
void gatherEdges(const ft_pose_opt_frame *F, FtPoseEdge *E) {
    const int nL = F->Nleft == -1 ? F->N : F->Nleft;
    for (int i = 0; i < F->N; i++) {
        if (!F->has_point[i]) continue;
        const bool right = i >= nL;
        const ft_keypoint &kp = right ? F->keys_right[i - nL] : F->keys[i];
        const float ur = (F->Nleft == -1 && F->uright) ? F->uright[i] : -1.f;
        memcpy(E->X, F->world_pos + 3 * (size_t)i, sizeof E->X);
        E->obs[0] = kp.x, E->obs[1] = kp.y;
        E->kind = right ? 1 : (F->Nleft == -1 && !(ur < 0)) ? 2 : 0;  // if (pFrame->mvuRight[i] < 0) mono else stereo
        E->obs[2] = E->kind == 2 ? ur : 0.f;
        E->w = F->inv_level_sigma2[kp.octave];
        E++;
    }
}

}  // namespace

extern "C" int ft_pose_optimization(ft_context *ctx, int n_frames, const ft_pose_opt_frame *frames, ft_se3 *Tcw_out, uint8_t *const *outlier,
                                    int *n_inliers, ft_pose_opt_trace *trace) {
    const std::string who = FN;
    FT_REQUIRE(ctx, who + ": null context");
    FT_REQUIRE(n_frames >= 0 && n_frames < (1 << 16), who + ": n_frames out of range");
    FT_REQUIRE(n_frames == 0 || (frames && Tcw_out && outlier && n_inliers), who + ": null argument");
    std::vector<int> nE((size_t)n_frames);
    int nJobs = 0;
    size_t totalEdges = 0;
    for (int f = 0; f < n_frames; f++) {
        const int rc = checkPoseOptFrame(who + ": frame " + std::to_string(f) + ": ", frames + f, outlier[f], &nE[f]);
        if (rc != FT_OK) return rc;
        if (nE[f] > FT_POSE_OPT_MAX_EDGES) {
            ft_set_error(who + ": frame " + std::to_string(f) + " has " + std::to_string(nE[f]) + " correspondences, more than the " +
                         std::to_string(FT_POSE_OPT_MAX_EDGES) + " a frame may hold");
            return FT_ERR_CAPACITY;
        }
        if (nE[f] >= 3) nJobs++, totalEdges += (size_t)nE[f];
    }
    ft_pose_opt_trace none;
    memset(&none, 0, sizeof none);
    auto clearFlags = [&](int f) {  // pFrame->mvbOutlier[i] = false with every edge (:869, 897, 938, 968)
        for (int i = 0; i < frames[f].N; i++)
            if (frames[f].has_point[i]) outlier[f][i] = 0;
    };
    if (nJobs == 0) {
        for (int f = 0; f < n_frames; f++) {
            clearFlags(f);
            Tcw_out[f] = frames[f].Tcw;
            n_inliers[f] = 0;
            if (trace) trace[f] = none;
        }
        return FT_OK;
    }
    int rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    // the arena: jobs | edges of all jobs || chi2 and level of the edges (device only) | results | outlier flags of the edges
    Arena a;
    const size_t oJobs = a.take(sizeof(FtPoseOptJob) * (size_t)nJobs);
    const size_t oEdges = a.take(sizeof(FtPoseEdge) * totalEdges);
    const size_t inputEnd = a.off;
    const size_t oWork = a.take(5 * totalEdges + 8 * (size_t)nJobs);
    const size_t oOut = a.take(sizeof(FtPoseOptOut) * (size_t)nJobs);
    const size_t oFlags = a.take(totalEdges);
    rc = ft_ensure_scratch(ctx, a.off, a.off);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    FtPoseOptJob *jobs = (FtPoseOptJob *)(pin + oJobs);
    FtPoseEdge *edges = (FtPoseEdge *)(pin + oEdges);
    size_t e0 = 0, w0 = oWork;
    for (int f = 0, j = 0; f < n_frames; f++) {
        if (nE[f] < 3) continue;
        const ft_pose_opt_frame *F = frames + f;
        FtPoseOptJob &J = jobs[j];
        memset(&J, 0, sizeof J);
        J.edges = (unsigned)(oEdges + sizeof(FtPoseEdge) * e0);
        J.work = (unsigned)w0;
        J.out = (unsigned)(oOut + sizeof(FtPoseOptOut) * (size_t)j);
        J.flags = (unsigned)(oFlags + e0);
        J.nE = nE[f];
        J.model = F->cam_model;
        J.twoCam = F->Nleft != -1;
        memcpy(J.cam, F->cam, sizeof J.cam);
        memcpy(J.cam2, F->cam2, sizeof J.cam2);
        J.bf = F->mbf;
        memcpy(J.q, F->Tcw.q, sizeof J.q);
        memcpy(J.t, F->Tcw.t, sizeof J.t);
        J.trlQ[3] = 1.f;
        if (J.twoCam) memcpy(J.trlQ, F->Trl.q, sizeof J.trlQ), memcpy(J.trlT, F->Trl.t, sizeof J.trlT);
        gatherEdges(F, edges + e0);
        e0 += (size_t)nE[f];
        w0 += (5 * (size_t)nE[f] + 7) & ~(size_t)7;  // the float chi2 of the next job stays aligned
        j++;
    }
    FtPoseOptCall T;
    T.arena = dev;
    T.jobs = (unsigned)oJobs;
    T.nJobs = nJobs;
    hipStream_t st = ctx->stream;
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, inputEnd);  // one copy: the block is contiguous
    C.launch("kernel.pose_opt", [&] { return ft_launch_pose_opt(st, T); });
    rc = C.down(oOut, a.off);
    if (rc != FT_OK) return rc;
    e0 = 0;
    for (int f = 0, j = 0; f < n_frames; f++) {
        const ft_pose_opt_frame *F = frames + f;
        if (nE[f] < 3) {
            clearFlags(f);
            Tcw_out[f] = F->Tcw;
            n_inliers[f] = 0;
            if (trace) trace[f] = none;
            continue;
        }
        const FtPoseOptOut *O = (const FtPoseOptOut *)(pin + oOut) + j;
        const uint8_t *fl = pin + oFlags + e0;
        for (int i = 0, k = 0; i < F->N; i++)
            if (F->has_point[i]) outlier[f][i] = fl[k++];
        memcpy(Tcw_out[f].q, O->q, sizeof O->q);
        memcpy(Tcw_out[f].t, O->t, sizeof O->t);
        n_inliers[f] = O->ret;
        if (trace) {
            memcpy(trace[f].iterations, O->iterations, sizeof O->iterations);
            memcpy(trace[f].rejected, O->rejected, sizeof O->rejected);
            memcpy(trace[f].chi2, O->chi, sizeof O->chi);
        }
        e0 += (size_t)nE[f];
        j++;
    }
    ctx->addStat("pose_optimization.total", tAll.ms());
    ctx->addStat("pose_optimization.launches", C.launches);
    return FT_OK;
}

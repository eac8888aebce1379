// ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (src/ORBmatcher.cc:322-524) as Tracking::Relocalization calls it
// (src/Tracking.cc:3839-3860): here one frame against all the candidate keyframes of a call.  The host packs the frame's side and
// every candidate's into one pinned block together with the -1 of the rows and enqueues: the block up, k_bow_cand_match,
// k_bow_cand_finish (kernels_bow_cand.hip), the results down - and waits once.  Nothing of that sequence depends on the number
// of candidates or on what they hold.  Descriptors of the frame that are resident on the device are read where they are.
#include <vector>

#include "search_host.h"

static const char *const FN = "ft_search_by_bow_candidates";

extern "C" {

int ft_search_by_bow_candidates(ft_context *ctx, const ft_bow_side *frame, int frame_nleft, int frame_descriptors_on_device, int n_keyframes,
                                const ft_bow_candidate *keyframes, float nn_ratio, int check_orientation, int *matches, int *n_matches) {
    FT_REQUIRE(ctx && frame, "ft_search_by_bow_candidates: null argument");
    FT_REQUIRE(n_keyframes >= 0 && n_keyframes < (1 << 16), "ft_search_by_bow_candidates: n_keyframes out of range");
    FT_REQUIRE(n_keyframes == 0 || (keyframes && n_matches), "ft_search_by_bow_candidates: null keyframes or n_matches");
    const bool ori = check_orientation != 0, resident = frame_descriptors_on_device != 0;
    // a frame feature sits under one node: what makes the nodes, and with them the waves of a candidate, independent
    int rc = checkBowSide(frame, "frame", FN, true);
    if (rc != FT_OK) return rc;
    const int N = frame->n;
    FT_REQUIRE(frame_nleft >= -1 && frame_nleft <= N, "ft_search_by_bow_candidates: frame_nleft out of range");
    FT_REQUIRE(!ori || N == 0 || frame->angles, "ft_search_by_bow_candidates: frame: check_orientation needs the keypoint angles");
    for (int k = 0; k < n_keyframes; k++) {
        const std::string who = "keyframe [" + std::to_string(k) + "]";
        const ft_bow_side *s = &keyframes[k].side;
        rc = checkBowSide(s, who.c_str(), FN);
        if (rc != FT_OK) return rc;
        const std::string w = std::string(FN) + ": " + who + ": ";
        FT_REQUIRE(s->n == 0 || keyframes[k].has_point, w + "null has_point");
        FT_REQUIRE(!ori || s->n == 0 || s->angles, w + "check_orientation needs the keypoint angles");
    }
    FT_REQUIRE(N == 0 || n_keyframes == 0 || matches, "ft_search_by_bow_candidates: null matches");
    if (N == 0 || n_keyframes == 0) {
        for (int k = 0; k < n_keyframes; k++) n_matches[k] = 0;
        return FT_OK;
    }
    // the arena: frame side | candidates | jobs | matches (-1) || n_matches
    Arena a;
    const BowSideLayout LF = layoutBowSide(a, frame, false, !resident, ori);
    std::vector<BowSideLayout> LK((size_t)n_keyframes);
    for (int k = 0; k < n_keyframes; k++) LK[k] = layoutBowSide(a, &keyframes[k].side, true, true, ori);
    const size_t oJobs = a.take(sizeof(FtBowCandJob) * (size_t)n_keyframes);
    const size_t rows = 4 * (size_t)N * (size_t)n_keyframes;
    const size_t oMatches = a.take(rows);
    const size_t inputEnd = a.off;
    const size_t oCount = a.take(4 * (size_t)n_keyframes);
    if (a.off >= 0xffffffffull) {
        ft_set_error("ft_search_by_bow_candidates: the keyframes of one call exceed 4 GB");
        return FT_ERR_CAPACITY;
    }
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    rc = ft_ensure_scratch(ctx, a.off, a.off);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    FtBowCandCall T;
    memset(&T, 0, sizeof T);
    T.arena = dev;
    T.F = stageBowSide(frame, nullptr, LF, pin);
    T.frameDesc = resident ? frame->descriptors : dev + LF.desc;
    FtBowCandJob *jobs = (FtBowCandJob *)(pin + oJobs);
    for (int k = 0; k < n_keyframes; k++) {
        FtBowCandJob &J = jobs[k];
        J.K = stageBowSide(&keyframes[k].side, keyframes[k].has_point, LK[k], pin);
        J.matches = (unsigned)(oMatches + 4 * (size_t)N * k);
        T.maxNodes = std::max(T.maxNodes, J.K.fv.nNodes);
    }
    memset(pin + oMatches, 0xff, rows);  // everything the kernel does not write is -1
    T.jobs = (unsigned)oJobs;
    T.nMatches = (unsigned)oCount;
    T.nCandidates = n_keyframes;
    T.nLeft = frame_nleft;
    T.checkOrientation = ori;
    T.nnRatio = nn_ratio;
    hipStream_t st = ctx->stream;
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, inputEnd);  // one copy: the block is contiguous
    C.launch("kernel.bow_cand_match", [&] { return ft_launch_bow_cand_match(st, T); });
    C.launch("kernel.bow_cand_finish", [&] { return ft_launch_bow_cand_finish(st, T); });
    rc = C.down(oMatches, a.off);
    if (rc != FT_OK) return rc;
    memcpy(matches, pin + oMatches, rows);
    memcpy(n_matches, pin + oCount, 4 * (size_t)n_keyframes);
    ctx->addStat("search_by_bow_candidates.total", tAll.ms());
    ctx->addStat("search_by_bow_candidates.launches", C.launches);
    ctx->addStat("search_by_bow_candidates.up_bytes", (double)inputEnd);
    return FT_OK;
}

}  // extern "C"

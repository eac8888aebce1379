// ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (src/ORBmatcher.cc:322-524) as Tracking::Relocalization calls it
// (src/Tracking.cc:3839-3860): here one frame against all the candidate keyframes of a call.  The host packs the frame's side and
// every candidate's into one pinned block together with the -1 of the rows and enqueues: the block up, k_bow_cand_match,
// k_bow_cand_finish (kernels_bow_cand.hip), the results down - and waits once.  Nothing of that sequence depends on the number
// of candidates or on what they hold.  Descriptors of the frame that are resident on the device are read where they are.
#include <vector>

#include "search_host.h"

namespace {

const char *const FN = "ft_search_by_bow_candidates";

struct SideLayout {
    size_t nodes, offsets, feats, desc, hasPoint, angles;
    int total;  // FeatureVector entries
};

// has: the side's has_point, null for the frame; desc: whether the side's descriptors are staged in the arena
SideLayout layoutSide(Arena &a, const ft_bow_side *s, bool has, bool desc, bool angles) {
    SideLayout L;
    const size_t n = (size_t)std::max(s->n, 1), nn = (size_t)s->n_nodes;
    L.total = s->n_nodes ? s->fv_offsets[s->n_nodes] : 0;
    L.nodes = a.take(4 * std::max(nn, (size_t)1));
    L.offsets = a.take(4 * (nn + 1));
    L.feats = a.take(4 * (size_t)std::max(L.total, 1));
    L.desc = desc ? a.take(32 * n) : 0;
    L.hasPoint = has ? a.take(n) : 0;
    L.angles = angles ? a.take(4 * n) : 0;
    return L;
}

FtBowCandSide stageSide(const ft_bow_side *s, const uint8_t *has, bool desc, const SideLayout &L, bool angles, uint8_t *pin) {
    const size_t n = (size_t)s->n, nn = (size_t)s->n_nodes;
    if (n) {
        if (desc) memcpy(pin + L.desc, s->descriptors, 32 * n);
        if (has) memcpy(pin + L.hasPoint, has, n);
        if (angles) memcpy(pin + L.angles, s->angles, 4 * n);
    }
    if (nn) {
        memcpy(pin + L.nodes, s->fv_nodes, 4 * nn);
        memcpy(pin + L.offsets, s->fv_offsets, 4 * (nn + 1));
        if (L.total) memcpy(pin + L.feats, s->fv_features, 4 * (size_t)L.total);
    } else {
        memset(pin + L.offsets, 0, 4);
    }
    FtBowCandSide D;
    D.n = s->n;
    D.nNodes = s->n_nodes;
    D.nodes = (unsigned)L.nodes;
    D.offsets = (unsigned)L.offsets;
    D.feats = (unsigned)L.feats;
    D.desc = (unsigned)L.desc;
    D.hasPoint = (unsigned)L.hasPoint;
    D.angles = (unsigned)L.angles;
    return D;
}

}  // namespace

extern "C" {

int ft_search_by_bow_candidates(ft_context *ctx, const ft_bow_side *frame, int frame_nleft, int frame_descriptors_on_device, int n_keyframes,
                                const ft_bow_candidate *keyframes, float nn_ratio, int check_orientation, int *matches, int *n_matches) {
    FT_REQUIRE(ctx && frame, "ft_search_by_bow_candidates: null argument");
    FT_REQUIRE(n_keyframes >= 0 && n_keyframes < (1 << 16), "ft_search_by_bow_candidates: n_keyframes out of range");
    FT_REQUIRE(n_keyframes == 0 || (keyframes && n_matches), "ft_search_by_bow_candidates: null keyframes or n_matches");
    const bool ori = check_orientation != 0, resident = frame_descriptors_on_device != 0;
    int rc = checkBowSide(frame, "frame", FN);
    if (rc != FT_OK) return rc;
    const int N = frame->n;
    FT_REQUIRE(frame_nleft >= -1 && frame_nleft <= N, "ft_search_by_bow_candidates: frame_nleft out of range");
    FT_REQUIRE(!ori || N == 0 || frame->angles, "ft_search_by_bow_candidates: frame: check_orientation needs the keypoint angles");
    {   // a frame feature sits under one node: what makes the nodes, and with them the waves of a candidate, independent
        std::vector<uint8_t> seen((size_t)N, 0);
        const int total = frame->n_nodes ? frame->fv_offsets[frame->n_nodes] : 0;
        for (int e = 0; e < total; e++) {
            FT_REQUIRE(!seen[frame->fv_features[e]], "ft_search_by_bow_candidates: frame: a feature is listed twice");
            seen[frame->fv_features[e]] = 1;
        }
    }
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
    const SideLayout LF = layoutSide(a, frame, false, !resident, ori);
    std::vector<SideLayout> LK((size_t)n_keyframes);
    for (int k = 0; k < n_keyframes; k++) LK[k] = layoutSide(a, &keyframes[k].side, true, true, ori);
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
    T.F = stageSide(frame, nullptr, !resident, LF, ori, pin);
    T.frameDesc = resident ? frame->descriptors : dev + LF.desc;
    FtBowCandJob *jobs = (FtBowCandJob *)(pin + oJobs);
    for (int k = 0; k < n_keyframes; k++) {
        FtBowCandJob &J = jobs[k];
        J.K = stageSide(&keyframes[k].side, keyframes[k].has_point, true, LK[k], ori, pin);
        J.matches = (unsigned)(oMatches + 4 * (size_t)N * k);
        T.maxNodes = std::max(T.maxNodes, J.K.nNodes);
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

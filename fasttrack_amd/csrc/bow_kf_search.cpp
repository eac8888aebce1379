// ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (src/ORBmatcher.cc:864-1004), the first step of
// LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:657-668): here keyframe 1 against all the keyframes of a call.  The
// host packs every side into one pinned block together with the -1 of matches12 and the 0 of the claim flags and enqueues: the block
// up, k_bow_kf_match, k_bow_kf_finish (kernels_bow_kf.hip), the results down - and waits once.  Nothing of that sequence depends on
// the number of keyframes or on what they hold.
#include <vector>

#include "search_host.h"

namespace {

const char *const FN = "ft_search_by_bow_keyframes";

struct SideLayout {
    size_t nodes, offsets, feats, desc, hasPoint, angles;
    int total;  // FeatureVector entries
};

int checkKeyframe(const ft_bow_keyframe *k, const std::string &who, bool needAngles, std::vector<uint8_t> &seen) {
    const ft_bow_side *s = &k->side;
    int rc = checkBowSide(s, who.c_str(), FN);
    if (rc != FT_OK) return rc;
    const std::string w = std::string(FN) + ": " + who + ": ";
    FT_REQUIRE(s->n == 0 || k->has_point, w + "null has_point");
    FT_REQUIRE(k->n_left >= -1 && k->n_left <= s->n, w + "n_left out of range");
    FT_REQUIRE(k->n_left == -1 || (k->n_un >= 0 && k->n_un <= s->n), w + "n_un out of range");
    FT_REQUIRE(!needAngles || s->n == 0 || s->angles, w + "check_orientation needs the keypoint angles");
    const int total = s->n_nodes ? s->fv_offsets[s->n_nodes] : 0;
    seen.assign((size_t)s->n, 0);
    for (int e = 0; e < total; e++) {
        FT_REQUIRE(!seen[s->fv_features[e]], w + "a feature is listed twice");  // a FeatureVector holds a feature under one node
        seen[s->fv_features[e]] = 1;
    }
    return FT_OK;
}

SideLayout layoutSide(Arena &a, const ft_bow_keyframe *k, bool angles) {
    const ft_bow_side *s = &k->side;
    SideLayout L;
    const size_t n = (size_t)std::max(s->n, 1), nn = (size_t)s->n_nodes;
    L.total = s->n_nodes ? s->fv_offsets[s->n_nodes] : 0;
    L.nodes = a.take(4 * std::max(nn, (size_t)1));
    L.offsets = a.take(4 * (nn + 1));
    L.feats = a.take(4 * (size_t)std::max(L.total, 1));
    L.desc = a.take(32 * n);
    L.hasPoint = a.take(n);
    L.angles = angles ? a.take(4 * n) : 0;
    return L;
}

FtBowKfSide stageSide(const ft_bow_keyframe *k, const SideLayout &L, bool angles, uint8_t *pin) {
    const ft_bow_side *s = &k->side;
    const size_t n = (size_t)s->n, nn = (size_t)s->n_nodes;
    if (n) {
        memcpy(pin + L.desc, s->descriptors, 32 * n);
        memcpy(pin + L.hasPoint, k->has_point, n);
        if (angles) memcpy(pin + L.angles, s->angles, 4 * n);
    }
    if (nn) {
        memcpy(pin + L.nodes, s->fv_nodes, 4 * nn);
        memcpy(pin + L.offsets, s->fv_offsets, 4 * (nn + 1));
        if (L.total) memcpy(pin + L.feats, s->fv_features, 4 * (size_t)L.total);
    } else {
        memset(pin + L.offsets, 0, 4);
    }
    FtBowKfSide D;
    D.n = s->n;
    D.nNodes = s->n_nodes;
    D.nLeft = k->n_left;
    D.nUn = k->n_left == -1 ? s->n : k->n_un;
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

int ft_search_by_bow_keyframes(ft_context *ctx, const ft_bow_keyframe *kf1, int n_keyframes, const ft_bow_keyframe *kf2, float nn_ratio,
                               int check_orientation, int *matches12, int *n_matches) {
    FT_REQUIRE(ctx && kf1, "ft_search_by_bow_keyframes: null argument");
    FT_REQUIRE(n_keyframes >= 0 && n_keyframes < (1 << 16), "ft_search_by_bow_keyframes: n_keyframes out of range");
    FT_REQUIRE(n_keyframes == 0 || (kf2 && n_matches), "ft_search_by_bow_keyframes: null keyframes or n_matches");
    const bool ori = check_orientation != 0;
    std::vector<uint8_t> seen;
    int rc = checkKeyframe(kf1, "keyframe 1", ori, seen);
    if (rc != FT_OK) return rc;
    for (int k = 0; k < n_keyframes; k++) {
        rc = checkKeyframe(kf2 + k, "keyframe 2 [" + std::to_string(k) + "]", ori, seen);
        if (rc != FT_OK) return rc;
    }
    const int n1 = kf1->side.n;
    FT_REQUIRE(n1 == 0 || n_keyframes == 0 || matches12, "ft_search_by_bow_keyframes: null matches12");
    if (n1 == 0 || n_keyframes == 0) {
        for (int k = 0; k < n_keyframes; k++) n_matches[k] = 0;
        return FT_OK;
    }
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    // the arena: keyframe 1 | the keyframes 2 | jobs | claim flags (0) | matches12 (-1) || n_matches
    Arena a;
    const SideLayout L1 = layoutSide(a, kf1, ori);
    std::vector<SideLayout> L2((size_t)n_keyframes);
    for (int k = 0; k < n_keyframes; k++) L2[k] = layoutSide(a, kf2 + k, ori);
    const size_t oJobs = a.take(sizeof(FtBowKfJob) * (size_t)n_keyframes);
    const size_t oClaimed = a.off;
    std::vector<size_t> oClaim((size_t)n_keyframes);
    for (int k = 0; k < n_keyframes; k++) oClaim[k] = a.take(4 * (size_t)std::max(kf2[k].side.n, 1));
    const size_t rows = 4 * (size_t)n1 * (size_t)n_keyframes;
    const size_t oMatches = a.take(rows);
    const size_t inputEnd = a.off;
    const size_t oCount = a.take(4 * (size_t)n_keyframes);
    if (a.off >= 0xffffffffull) {
        ft_set_error("ft_search_by_bow_keyframes: the keyframes of one call exceed 4 GB");
        return FT_ERR_CAPACITY;
    }
    rc = ft_ensure_scratch(ctx, a.off, a.off);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    FtBowKfCall T;
    memset(&T, 0, sizeof T);
    T.arena = dev;
    T.K1 = stageSide(kf1, L1, ori, pin);
    FtBowKfJob *jobs = (FtBowKfJob *)(pin + oJobs);
    for (int k = 0; k < n_keyframes; k++) {
        FtBowKfJob &J = jobs[k];
        J.K2 = stageSide(kf2 + k, L2[k], ori, pin);
        J.matches = (unsigned)(oMatches + 4 * (size_t)n1 * k);
        J.claimed = (unsigned)oClaim[k];
    }
    memset(pin + oClaimed, 0, oMatches - oClaimed);
    memset(pin + oMatches, 0xff, rows);  // everything the kernel does not write is -1
    T.jobs = (unsigned)oJobs;
    T.nMatches = (unsigned)oCount;
    T.nNeighbours = n_keyframes;
    T.checkOrientation = ori;
    T.nnRatio = nn_ratio;
    hipStream_t st = ctx->stream;
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, inputEnd);  // one copy: the block is contiguous
    C.launch("kernel.bow_kf_match", [&] { return ft_launch_bow_kf_match(st, T); });
    C.launch("kernel.bow_kf_finish", [&] { return ft_launch_bow_kf_finish(st, T); });
    rc = C.down(oMatches, a.off);
    if (rc != FT_OK) return rc;
    memcpy(matches12, pin + oMatches, rows);
    memcpy(n_matches, pin + oCount, 4 * (size_t)n_keyframes);
    ctx->addStat("search_by_bow_keyframes.total", tAll.ms());
    ctx->addStat("search_by_bow_keyframes.launches", C.launches);
    return FT_OK;
}

}  // extern "C"

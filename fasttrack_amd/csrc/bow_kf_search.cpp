// ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (src/ORBmatcher.cc:864-1004), the first step of
// LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:657-668): here keyframe 1 against all the keyframes of a call.  The
// host packs every side into one pinned block together with the -1 of matches12 and the 0 of the claim flags and enqueues: the block
// up, k_bow_kf_match, k_bow_kf_finish (kernels_bow_kf.hip), the results down - and waits once.  Nothing of that sequence depends on
// the number of keyframes or on what they hold.
#include <vector>

#include "search_host.h"

namespace {

const char *const FN = "ft_search_by_bow_keyframes";

int checkKeyframe(const ft_bow_keyframe *k, const std::string &who, bool needAngles) {
    const ft_bow_side *s = &k->side;
    int rc = checkBowSide(s, who.c_str(), FN, true);  // a FeatureVector holds a feature under one node
    if (rc != FT_OK) return rc;
    const std::string w = std::string(FN) + ": " + who + ": ";
    FT_REQUIRE(s->n == 0 || k->has_point, w + "null has_point");
    FT_REQUIRE(k->n_left >= -1 && k->n_left <= s->n, w + "n_left out of range");
    FT_REQUIRE(k->n_left == -1 || (k->n_un >= 0 && k->n_un <= s->n), w + "n_un out of range");
    FT_REQUIRE(!needAngles || s->n == 0 || s->angles, w + "check_orientation needs the keypoint angles");
    return FT_OK;
}

// the side of a keyframe: with has_point and descriptors, and what KeyFrame::NLeft / mvKeysUn.size() say of a second camera
FtBowArenaSide stageKeyframe(const ft_bow_keyframe *k, const BowSideLayout &L, uint8_t *pin) {
    FtBowArenaSide D = stageBowSide(&k->side, k->has_point, L, pin);
    D.nLeft = k->n_left;
    if (k->n_left != -1) D.nUn = k->n_un;
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
    int rc = checkKeyframe(kf1, "keyframe 1", ori);
    if (rc != FT_OK) return rc;
    for (int k = 0; k < n_keyframes; k++) {
        rc = checkKeyframe(kf2 + k, "keyframe 2 [" + std::to_string(k) + "]", ori);
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
    const BowSideLayout L1 = layoutBowSide(a, &kf1->side, true, true, ori);
    std::vector<BowSideLayout> L2((size_t)n_keyframes);
    for (int k = 0; k < n_keyframes; k++) L2[k] = layoutBowSide(a, &kf2[k].side, true, true, ori);
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
    T.K1 = stageKeyframe(kf1, L1, pin);
    FtBowKfJob *jobs = (FtBowKfJob *)(pin + oJobs);
    for (int k = 0; k < n_keyframes; k++) {
        FtBowKfJob &J = jobs[k];
        J.K2 = stageKeyframe(kf2 + k, L2[k], pin);
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

// ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (src/ORBmatcher.cc:1006-1245), the matcher
// LocalMapping::CreateNewMapPoints calls once per covisible neighbour of a new keyframe (src/LocalMapping.cc:388-466): here
// keyframe 1 against all its neighbours in one call.  The host packs every side and pair into one pinned block and enqueues: the
// block up, k_triang_match, k_triang_finish (kernels_triang.hip), the results down - and waits once.  Nothing of that sequence
// depends on the number of neighbours or on what the keyframes hold.
#include <vector>

#include "search_host.h"

namespace {

struct SideLayout {
    size_t keys, desc, nodes, offsets, feats, hasPoint, uright, sf, sigma2;
    int total;  // FeatureVector entries
};

int checkTriangSide(const ft_triang_keyframe *s, const std::string &who, std::vector<uint8_t> &seen) {
    const std::string w = "ft_search_for_triangulation: " + who + ": ";
    FT_REQUIRE(s->n >= 0 && s->n < (1 << 20) && s->n_nodes >= 0, w + "count out of range");
    FT_REQUIRE(s->n_left >= -1 && s->n_left <= s->n, w + "n_left out of range");
    FT_REQUIRE(s->cam_model == 0 || s->cam_model == 1, w + "unknown camera model");
    FT_REQUIRE(!(s->cam_model == 0 && s->two_cameras), w + "a pinhole keyframe with two cameras");
    FT_REQUIRE(s->scale_factors && s->level_sigma2 && s->nlevels >= 1 && s->nlevels <= FT_MAX_LEVELS, w + "scale factors / level sigmas missing");
    FT_REQUIRE(s->n == 0 || (s->keys && s->descriptors && s->has_point), w + "keypoints, descriptors or has_point are null");
    for (int i = 0; i < s->n; i++) FT_REQUIRE(s->keys[i].octave >= 0 && s->keys[i].octave < s->nlevels, w + "keypoint octave outside [0, nlevels)");
    if (s->n_nodes == 0) return FT_OK;
    FT_REQUIRE(s->fv_nodes && s->fv_offsets, w + "null feature vector");
    FT_REQUIRE(s->fv_offsets[0] == 0, w + "fv_offsets[0] != 0");
    for (int j = 0; j < s->n_nodes; j++) {
        FT_REQUIRE(s->fv_offsets[j + 1] >= s->fv_offsets[j], w + "fv_offsets not ascending");
        FT_REQUIRE(j == 0 || s->fv_nodes[j] > s->fv_nodes[j - 1], w + "fv_nodes not strictly ascending");
    }
    const int total = s->fv_offsets[s->n_nodes];
    FT_REQUIRE(total <= s->n, w + "more feature-vector entries than features");
    FT_REQUIRE(total == 0 || s->fv_features, w + "null fv_features");
    seen.assign((size_t)s->n, 0);
    for (int e = 0; e < total; e++) {
        FT_REQUIRE(s->fv_features[e] < (unsigned)s->n, w + "feature index out of range");
        FT_REQUIRE(!seen[s->fv_features[e]], w + "a feature is listed twice");  // a FeatureVector holds a feature under one node
        seen[s->fv_features[e]] = 1;
    }
    return FT_OK;
}

SideLayout layoutSide(Arena &a, const ft_triang_keyframe *s) {
    SideLayout L;
    const size_t n = (size_t)std::max(s->n, 1), nn = (size_t)s->n_nodes;
    L.total = s->n_nodes ? s->fv_offsets[s->n_nodes] : 0;
    L.keys = a.take(sizeof(ft_keypoint) * n);
    L.desc = a.take(32 * n);
    L.nodes = a.take(4 * std::max(nn, (size_t)1));
    L.offsets = a.take(4 * (nn + 1));
    L.feats = a.take(4 * (size_t)std::max(L.total, 1));
    L.hasPoint = a.take(n);
    L.uright = s->uright ? a.take(4 * n) : 0;
    L.sf = a.take(4 * FT_MAX_LEVELS);
    L.sigma2 = a.take(4 * FT_MAX_LEVELS);
    return L;
}

FtTriangSide stageSide(const ft_triang_keyframe *s, const SideLayout &L, uint8_t *pin) {
    const size_t n = (size_t)s->n, nn = (size_t)s->n_nodes;
    if (n) {
        memcpy(pin + L.keys, s->keys, sizeof(ft_keypoint) * n);
        memcpy(pin + L.desc, s->descriptors, 32 * n);
        memcpy(pin + L.hasPoint, s->has_point, n);
        if (s->uright) memcpy(pin + L.uright, s->uright, 4 * n);
    }
    if (nn) {
        memcpy(pin + L.nodes, s->fv_nodes, 4 * nn);
        memcpy(pin + L.offsets, s->fv_offsets, 4 * (nn + 1));
        if (L.total) memcpy(pin + L.feats, s->fv_features, 4 * (size_t)L.total);
    } else {
        memset(pin + L.offsets, 0, 4);
    }
    memcpy(pin + L.sf, s->scale_factors, 4 * (size_t)s->nlevels);
    memcpy(pin + L.sigma2, s->level_sigma2, 4 * (size_t)s->nlevels);
    FtTriangSide D;
    D.n = s->n;
    D.nLeft = s->n_left;
    D.nNodes = s->n_nodes;
    D.keys = (unsigned)L.keys;
    D.desc = (unsigned)L.desc;
    D.nodes = (unsigned)L.nodes;
    D.offsets = (unsigned)L.offsets;
    D.feats = (unsigned)L.feats;
    D.hasPoint = (unsigned)L.hasPoint;
    D.uright = s->uright ? (unsigned)L.uright : FT_TRIANG_NONE;
    D.sf = (unsigned)L.sf;
    D.sigma2 = (unsigned)L.sigma2;
    memcpy(D.cam[0], s->cam, sizeof D.cam[0]);
    memcpy(D.cam[1], s->cam2, sizeof D.cam[1]);
    return D;
}

}  // namespace

extern "C" {

int ft_search_for_triangulation(ft_context *ctx, const ft_triang_keyframe *kf1, int n_neighbours, const ft_triang_keyframe *kf2,
                                const ft_triang_pair *pairs, int only_stereo, int coarse, int check_orientation, int *matches12,
                                int *n_matches, int *best_dist) {
    FT_REQUIRE(ctx && kf1, "ft_search_for_triangulation: null argument");
    FT_REQUIRE(n_neighbours >= 0 && n_neighbours < (1 << 16), "ft_search_for_triangulation: n_neighbours out of range");
    FT_REQUIRE(n_neighbours == 0 || (kf2 && pairs && n_matches), "ft_search_for_triangulation: null neighbours, pairs or n_matches");
    std::vector<uint8_t> seen;
    int rc = checkTriangSide(kf1, "keyframe 1", seen);
    if (rc != FT_OK) return rc;
    for (int k = 0; k < n_neighbours; k++) {
        rc = checkTriangSide(kf2 + k, "neighbour " + std::to_string(k), seen);
        if (rc != FT_OK) return rc;
        // the reference reads an uninitialised R12 when only one of the two keyframes has a second camera (:1027-1039, :1135)
        FT_REQUIRE(!kf2[k].two_cameras == !kf1->two_cameras && kf2[k].cam_model == kf1->cam_model,
                   "ft_search_for_triangulation: the keyframes of a call differ in two_cameras or in the camera model");
    }
    const int n1 = kf1->n;
    FT_REQUIRE(n1 == 0 || n_neighbours == 0 || matches12, "ft_search_for_triangulation: null matches12");
    if (n1 == 0 || n_neighbours == 0) {
        for (int k = 0; k < n_neighbours; k++) n_matches[k] = 0;
        return FT_OK;
    }
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    // the arena: keyframe 1 | its record | nodeOf | neighbour sides | jobs || matches12 | n_matches | best_dist
    Arena a;
    const SideLayout L1 = layoutSide(a, kf1);
    const size_t oK1 = a.take(sizeof(FtTriangSide));
    const size_t oNodeOf = a.take(4 * (size_t)n1);
    std::vector<SideLayout> L2((size_t)n_neighbours);
    for (int k = 0; k < n_neighbours; k++) L2[k] = layoutSide(a, kf2 + k);
    const size_t oJobs = a.take(sizeof(FtTriangJob) * (size_t)n_neighbours);
    const size_t inputEnd = a.off;
    const size_t rows = 4 * (size_t)n1 * (size_t)n_neighbours;
    const size_t oMatches = a.take(rows);
    const size_t oCount = a.take(4 * (size_t)n_neighbours);
    const size_t outEnd = a.off;  // without best_dist
    const size_t oBest = a.take(rows);
    if (a.off >= 0xffffffffull) {
        ft_set_error("ft_search_for_triangulation: the keyframes of one call exceed 4 GB");
        return FT_ERR_CAPACITY;
    }
    rc = ft_ensure_scratch(ctx, a.off, a.off);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    FtTriangCall T;
    memset(&T, 0, sizeof T);
    T.arena = dev;
    T.K1 = stageSide(kf1, L1, pin);
    memcpy(pin + oK1, &T.K1, sizeof T.K1);
    T.k1 = (unsigned)oK1;
    {
        int *nodeOf = (int *)(pin + oNodeOf);
        for (int i = 0; i < n1; i++) nodeOf[i] = -1;
        for (int j = 0; j < kf1->n_nodes; j++)
            for (int e = kf1->fv_offsets[j]; e < kf1->fv_offsets[j + 1]; e++) nodeOf[kf1->fv_features[e]] = j;
    }
    T.nodeOf = (unsigned)oNodeOf;
    FtTriangJob *jobs = (FtTriangJob *)(pin + oJobs);
    for (int k = 0; k < n_neighbours; k++) {
        FtTriangJob &J = jobs[k];
        J.K2 = stageSide(kf2 + k, L2[k], pin);
        memcpy(J.ep, pairs[k].ep, sizeof J.ep);
        memcpy(J.F12, pairs[k].F12, sizeof J.F12);
        memcpy(J.R12, pairs[k].R12, sizeof J.R12);
        memcpy(J.t12, pairs[k].t12, sizeof J.t12);
        J.precision = pairs[k].kb8_precision;
        J.matches = (unsigned)(oMatches + 4 * (size_t)n1 * k);
        J.bestDist = (unsigned)(oBest + 4 * (size_t)n1 * k);
    }
    T.jobs = (unsigned)oJobs;
    T.nMatches = (unsigned)oCount;
    T.nNeighbours = n_neighbours;
    T.camModel = kf1->cam_model;
    T.twoCameras = kf1->two_cameras != 0;
    T.onlyStereo = only_stereo != 0;
    T.coarse = coarse != 0;
    T.checkOrientation = check_orientation != 0;
    hipStream_t st = ctx->stream;
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, inputEnd);  // one copy: the block is contiguous
    C.launch("kernel.triang_match", [&] { return ft_launch_triang_match(st, T); });
    C.launch("kernel.triang_finish", [&] { return ft_launch_triang_finish(st, T); });
    rc = C.down(oMatches, best_dist ? a.off : outEnd);
    if (rc != FT_OK) return rc;
    memcpy(matches12, pin + oMatches, rows);
    memcpy(n_matches, pin + oCount, 4 * (size_t)n_neighbours);
    if (best_dist) memcpy(best_dist, pin + oBest, rows);
    ctx->addStat("search_for_triangulation.total", tAll.ms());
    ctx->addStat("search_for_triangulation.launches", C.launches);
    return FT_OK;
}

}  // extern "C"

// ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (src/ORBmatcher.cc:1006-1245), the matcher
// LocalMapping::CreateNewMapPoints calls once per covisible neighbour of a new keyframe (src/LocalMapping.cc:388-466): here
// keyframe 1 against all its neighbours in one call.  The host packs every side and pair into one pinned block and enqueues: the
// block up, k_triang_match, k_triang_finish (kernels_triang.hip), the results down - and waits once.  Nothing of that sequence
// depends on the number of neighbours or on what the keyframes hold.
#include "triang_host.h"

extern "C" {

int ft_search_for_triangulation(ft_context *ctx, const ft_triang_keyframe *kf1, int n_neighbours, const ft_triang_keyframe *kf2,
                                const ft_triang_pair *pairs, int only_stereo, int coarse, int check_orientation, int *matches12,
                                int *n_matches, int *best_dist) {
    FT_REQUIRE(ctx && kf1, "ft_search_for_triangulation: null argument");
    FT_REQUIRE(n_neighbours >= 0 && n_neighbours < (1 << 16), "ft_search_for_triangulation: n_neighbours out of range");
    FT_REQUIRE(n_neighbours == 0 || (kf2 && pairs && n_matches), "ft_search_for_triangulation: null neighbours, pairs or n_matches");
    int rc = checkTriangCall("ft_search_for_triangulation", kf1, n_neighbours, kf2, true);
    if (rc != FT_OK) return rc;
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
    TriangBlock B;
    B.layout(a, kf1, n_neighbours, kf2, true);
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
    FtTriangJob *jobs = B.stage(kf1, n_neighbours, kf2, pairs, pin, dev, T);
    for (int k = 0; k < n_neighbours; k++) {
        jobs[k].matches = (unsigned)(oMatches + 4 * (size_t)n1 * k);
        jobs[k].bestDist = (unsigned)(oBest + 4 * (size_t)n1 * k);
    }
    T.nMatches = (unsigned)oCount;
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

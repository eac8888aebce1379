// The triangulation of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:483-692) behind ORBmatcher::SearchForTriangulation:
// ft_triangulate_new_points on host match rows (the block up, k_triang_points, the results down) and ft_search_and_triangulate,
// which runs the matcher's two launches and k_triang_points in one arena, the match rows staying on the device in between.  Both
// wait once, and nothing of either sequence depends on the number of neighbours.  The block of the keyframes is triang_host.h's;
// behind it: the geometry records, mvDepth and mvKeys where given, and the initial values of the two accumulated outputs
// (n_points = 0, first_neighbour = -1) - they go up with the inputs and come down with the outputs, so nothing is memset.
#include "triang_host.h"

namespace {

struct GeomLayout {
    size_t depth, keysRaw;
};

int checkGeometry(const std::string &w, const ft_triang_keyframe *s, const ft_newpoint_geometry *g) {
    if (g->depth || s->two_cameras || !s->uright) return FT_OK;
    for (int i = 0; i < s->n; i++) FT_REQUIRE(!(s->uright[i] >= 0), w + "a keypoint with uright >= 0 and depth == NULL");
    return FT_OK;
}

GeomLayout layoutGeometry(Arena &a, const ft_triang_keyframe *s, const ft_newpoint_geometry *g) {
    GeomLayout L;
    const size_t n = (size_t)std::max(s->n, 1);
    L.depth = g->depth ? a.take(4 * n) : 0;
    L.keysRaw = g->keys_raw ? a.take(sizeof(ft_keypoint) * n) : 0;
    return L;
}

FtNewPointSide stageGeometry(const ft_triang_keyframe *s, const ft_newpoint_geometry *g, const GeomLayout &L, uint8_t *pin) {
    FtNewPointSide D;
    memcpy(D.Tcw[0], g->Tcw, sizeof D.Tcw[0]);
    memcpy(D.Tcw[1], g->Tcw_right, sizeof D.Tcw[1]);
    memcpy(D.Ow[0], g->Ow, sizeof D.Ow[0]);
    memcpy(D.Ow[1], g->Ow_right, sizeof D.Ow[1]);
    memcpy(D.Rwc, g->Rwc, sizeof D.Rwc);
    memcpy(D.twc, g->twc, sizeof D.twc);
    D.fx = g->fx, D.fy = g->fy, D.cx = g->cx, D.cy = g->cy, D.invfx = g->invfx, D.invfy = g->invfy, D.mb = g->mb, D.mbf = g->mbf;
    D.precision = g->kb8_precision;
    D.depth = D.keysRaw = FT_TRIANG_NONE;
    if (g->depth) {
        if (s->n) memcpy(pin + L.depth, g->depth, 4 * (size_t)s->n);
        D.depth = (unsigned)L.depth;
    }
    if (g->keys_raw) {
        if (s->n) memcpy(pin + L.keysRaw, g->keys_raw, sizeof(ft_keypoint) * (size_t)s->n);
        D.keysRaw = (unsigned)L.keysRaw;
    }
    return D;
}

// both entry points: pairs == null is the stand-alone stage on the host rows matches_in
int newPoints(const char *fn, ft_context *ctx, const ft_triang_keyframe *kf1, const ft_newpoint_geometry *g1, int n_neighbours,
              const ft_triang_keyframe *kf2, const ft_newpoint_geometry *g2, const ft_triang_pair *pairs, const int *matches_in, int only_stereo,
              int coarse, int check_orientation, int inertial, int far_points, float th_far_points, float ratio_factor, int *matches12,
              int *n_matches, int *best_dist, int *status, float *x3d, int *n_points, int *first_neighbour) {
    const std::string who = fn;
    const bool search = pairs != nullptr;
    FT_REQUIRE(ctx && kf1 && g1, who + ": null argument");
    FT_REQUIRE(n_neighbours >= 0 && n_neighbours < (1 << 16), who + ": n_neighbours out of range");
    FT_REQUIRE(n_neighbours == 0 || (kf2 && g2 && n_points && (!search || n_matches)), who + ": null neighbours, geometry or counts");
    int rc = checkTriangCall(who, kf1, n_neighbours, kf2, search);
    if (rc != FT_OK) return rc;
    rc = checkGeometry(who + ": keyframe 1: ", kf1, g1);
    if (rc != FT_OK) return rc;
    for (int k = 0; k < n_neighbours; k++) {
        rc = checkGeometry(who + ": neighbour " + std::to_string(k) + ": ", kf2 + k, g2 + k);
        if (rc != FT_OK) return rc;
    }
    const int n1 = kf1->n;
    const bool empty = n1 == 0 || n_neighbours == 0;
    FT_REQUIRE(empty || (status && x3d && first_neighbour && (search ? matches12 != nullptr : matches_in != nullptr)), who + ": null rows");
    if (!search && !empty)
        for (int k = 0; k < n_neighbours; k++)
            for (int i = 0; i < n1; i++)
                FT_REQUIRE(matches_in[(size_t)k * n1 + i] < kf2[k].n, who + ": a matches12 entry >= the neighbour's feature count");
    if (empty) {
        for (int k = 0; k < n_neighbours; k++) {
            n_points[k] = 0;
            if (search) n_matches[k] = 0;
        }
        for (int i = 0; i < n1 && first_neighbour; i++) first_neighbour[i] = -1;
        return FT_OK;
    }
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    // the arena: the keyframes' block | geometry of keyframe 1 | depth, mvKeys | new-point jobs | (host match rows) | n_points |
    // first_neighbour || (matches12 | n_matches) | status | x3d | (best_dist).  Down comes n_points ... x3d or best_dist.
    Arena a;
    TriangBlock B;
    B.layout(a, kf1, n_neighbours, kf2, search);
    const size_t oG1 = a.take(sizeof(FtNewPointSide));
    const GeomLayout GL1 = layoutGeometry(a, kf1, g1);
    std::vector<GeomLayout> GL2((size_t)n_neighbours);
    for (int k = 0; k < n_neighbours; k++) GL2[k] = layoutGeometry(a, kf2 + k, g2 + k);
    const size_t oNewJobs = a.take(sizeof(FtNewPointJob) * (size_t)n_neighbours);
    const size_t rows = 4 * (size_t)n1 * (size_t)n_neighbours;
    const size_t oRowsIn = search ? 0 : a.take(rows);
    const size_t oPoints = a.take(4 * (size_t)n_neighbours);
    const size_t oFirst = a.take(4 * (size_t)n1);
    const size_t inputEnd = a.off;
    const size_t oMatches = search ? a.take(rows) : oRowsIn;
    const size_t oCount = search ? a.take(4 * (size_t)n_neighbours) : 0;
    const size_t oStatus = a.take(rows);
    const size_t oX3d = a.take(3 * rows);
    const size_t outEnd = a.off;  // without best_dist
    const size_t oBest = search ? a.take(rows) : 0;
    if (a.off >= 0xffffffffull) {
        ft_set_error(who + ": the keyframes of one call exceed 4 GB");
        return FT_ERR_CAPACITY;
    }
    rc = ft_ensure_scratch(ctx, a.off, a.off);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    FtTriangCall T;
    FtTriangJob *jobs = B.stage(kf1, n_neighbours, kf2, pairs, pin, dev, T);
    T.nMatches = (unsigned)oCount;
    T.onlyStereo = only_stereo != 0;
    T.coarse = coarse != 0;
    T.checkOrientation = check_orientation != 0;
    FtNewPointCall P;
    memset(&P, 0, sizeof P);
    const FtNewPointSide G1 = stageGeometry(kf1, g1, GL1, pin);
    memcpy(pin + oG1, &G1, sizeof G1);
    P.g1 = (unsigned)oG1;
    FtNewPointJob *nj = (FtNewPointJob *)(pin + oNewJobs);
    for (int k = 0; k < n_neighbours; k++) {
        jobs[k].matches = (unsigned)(oMatches + 4 * (size_t)n1 * k);
        jobs[k].bestDist = (unsigned)(oBest + 4 * (size_t)n1 * k);
        nj[k].G2 = stageGeometry(kf2 + k, g2 + k, GL2[k], pin);
        nj[k].status = (unsigned)(oStatus + 4 * (size_t)n1 * k);
        nj[k].x3d = (unsigned)(oX3d + 12 * (size_t)n1 * k);
    }
    P.jobs = (unsigned)oNewJobs;
    P.nPoints = (unsigned)oPoints;
    P.firstNeighbour = (unsigned)oFirst;
    P.inertial = inertial != 0;
    P.farPoints = far_points != 0;
    P.thFar = th_far_points;
    P.ratioFactor = ratio_factor;
    if (!search) memcpy(pin + oRowsIn, matches_in, rows);
    memset(pin + oPoints, 0, 4 * (size_t)n_neighbours);
    memset(pin + oFirst, 0xff, 4 * (size_t)n1);
    hipStream_t st = ctx->stream;
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, inputEnd);  // one copy: the block is contiguous
    if (search) {
        C.launch("kernel.triang_match", [&] { return ft_launch_triang_match(st, T); });
        C.launch("kernel.triang_finish", [&] { return ft_launch_triang_finish(st, T); });
    }
    C.launch("kernel.triang_points", [&] { return ft_launch_triang_points(st, T, P); });
    rc = C.down(oPoints, search && best_dist ? a.off : outEnd);
    if (rc != FT_OK) return rc;
    if (search) {
        memcpy(matches12, pin + oMatches, rows);
        memcpy(n_matches, pin + oCount, 4 * (size_t)n_neighbours);
        if (best_dist) memcpy(best_dist, pin + oBest, rows);
    }
    memcpy(status, pin + oStatus, rows);
    memcpy(x3d, pin + oX3d, 3 * rows);
    memcpy(n_points, pin + oPoints, 4 * (size_t)n_neighbours);
    memcpy(first_neighbour, pin + oFirst, 4 * (size_t)n1);
    ctx->addStat(search ? "search_and_triangulate.total" : "triangulate_new_points.total", tAll.ms());
    ctx->addStat(search ? "search_and_triangulate.launches" : "triangulate_new_points.launches", C.launches);
    return FT_OK;
}

}  // namespace

extern "C" {

int ft_triangulate_new_points(ft_context *ctx, const ft_triang_keyframe *kf1, const ft_newpoint_geometry *g1, int n_neighbours,
                              const ft_triang_keyframe *kf2, const ft_newpoint_geometry *g2, const int *matches12, int inertial, int far_points,
                              float th_far_points, float ratio_factor, int *status, float *x3d, int *n_points, int *first_neighbour) {
    return newPoints("ft_triangulate_new_points", ctx, kf1, g1, n_neighbours, kf2, g2, nullptr, matches12, 0, 0, 0, inertial, far_points,
                     th_far_points, ratio_factor, nullptr, nullptr, nullptr, status, x3d, n_points, first_neighbour);
}

int ft_search_and_triangulate(ft_context *ctx, const ft_triang_keyframe *kf1, const ft_newpoint_geometry *g1, int n_neighbours,
                              const ft_triang_keyframe *kf2, const ft_newpoint_geometry *g2, const ft_triang_pair *pairs, int only_stereo, int coarse,
                              int check_orientation, int inertial, int far_points, float th_far_points, float ratio_factor, int *matches12,
                              int *n_matches, int *best_dist, int *status, float *x3d, int *n_points, int *first_neighbour) {
    FT_REQUIRE(n_neighbours <= 0 || pairs, "ft_search_and_triangulate: null pairs");
    static const ft_triang_pair none = {};
    return newPoints("ft_search_and_triangulate", ctx, kf1, g1, n_neighbours, kf2, g2, pairs ? pairs : &none, nullptr, only_stereo, coarse,
                     check_orientation, inertial, far_points, th_far_points, ratio_factor, matches12, n_matches, best_dist, status, x3d,
                     n_points, first_neighbour);
}

}  // extern "C"

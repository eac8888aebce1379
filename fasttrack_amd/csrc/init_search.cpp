// ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:747-862), the matcher of Tracking::MonocularInitialization
// (src/Tracking.cc:2516-2549).  The host enqueues: vbPrevMatched up, k_init_prepare, k_init_candidates, k_init_resolve
// (kernels_init.hip), the results down - and waits once.  Nothing of that sequence depends on what the frames hold.
#include "search_host.h"

namespace {

struct InitLayout {
    size_t prev, rows, ordOfPos, idxOfOrd, top, segCount;  // inputs and tables
    size_t out, matches, prevOut, tail, dist, outEnd;      // what comes back: matches12 | vbPrevMatched | nmatches, counts | vMatchedDistance
    size_t seg;
};
InitLayout layoutInit(Arena &a, int N1, int N2, int cap1, int cap2, bool wantDist) {
    InitLayout L;
    const size_t c1 = (size_t)std::max(cap1, 1), c2 = (size_t)std::max(cap2, 1), n1 = (size_t)std::max(N1, 1);
    L.prev = a.take(8 * n1);
    L.rows = a.take(4 * c1);
    L.ordOfPos = a.take(4 * c2);
    L.idxOfOrd = a.take(4 * c2);
    L.top = a.take(4 * FT_INIT_TOP * c1);
    L.segCount = a.take(4 * c1);
    L.out = a.off;
    L.matches = a.take(4 * n1);
    L.prevOut = a.take(8 * n1);
    L.tail = a.take(64);
    L.dist = wantDist ? a.take(4 * (size_t)std::max(N2, 1)) : 0;
    L.outEnd = a.off;
    L.seg = a.take(4 * c1 * c2);
    return L;
}

// S: F2 (with its grid), keys1, desc1, N1, cap1, cap2 and the call's parameters are set; C: the arena of layout L and its pinned
// mirror, vbPrevMatched is on its way up to L.prev.
int runInitSearch(CallScope &C, FtInitSearch S, const InitLayout &L, float *prev_matched, int *matches12, int *n_matches,
                  int *matched_distance, int N2) {
    uint8_t *dev = C.dev, *pin = C.pin;
    const int N1 = S.N1;
    S.prev = (const float *)(dev + L.prev);
    S.rows = (int *)(dev + L.rows);
    S.ordOfPos = (int *)(dev + L.ordOfPos);
    S.idxOfOrd = (int *)(dev + L.idxOfOrd);
    S.top = (unsigned *)(dev + L.top);
    S.segCount = (int *)(dev + L.segCount);
    S.seg = (unsigned *)(dev + L.seg);
    S.matches12 = (int *)(dev + L.matches);
    S.prevOut = (float *)(dev + L.prevOut);
    S.nMatches = (int *)(dev + L.tail);
    S.counts = (int *)(dev + L.tail) + 4;
    S.matchedDist = matched_distance ? (int *)(dev + L.dist) : nullptr;
    C.launch("kernel.init_prepare", [&] { return ft_launch_init_prepare(C.st, S); });
    C.launch("kernel.init_candidates", [&] { return ft_launch_init_candidates(C.st, S); });
    C.launch("kernel.init_resolve", [&] { return ft_launch_init_resolve(C.st, S); });
    const int rc = C.down(L.out, L.outEnd);
    if (rc != FT_OK) return rc;
    const int *tail = (const int *)(pin + L.tail);
    FT_REQUIRE(tail[6] == 0, "SearchForInitialization: the keypoint octaves on the device differ from the host's copy of the frame");
    memcpy(matches12, pin + L.matches, 4 * (size_t)N1);
    memcpy(prev_matched, pin + L.prevOut, 8 * (size_t)N1);
    if (matched_distance) memcpy(matched_distance, pin + L.dist, 4 * (size_t)N2);
    if (n_matches) *n_matches = tail[0];
    return FT_OK;
}

int checkInitCaps(int cap1, int cap2) {
    if (cap1 >= 0xffff || cap2 >= (1 << FT_INIT_ORD_BITS) || 4 * ((size_t)cap1 + (size_t)cap2) > FT_INIT_MAX_LDS) {
        ft_set_error("SearchForInitialization: too many level-0 keypoints (the tables of the resolution hold 38400 of both frames together)");
        return FT_ERR_CAPACITY;
    }
    return FT_OK;
}
}  // namespace

extern "C" {

int ft_search_for_initialization(ft_context *ctx, const ft_frame_view *F1, const ft_frame_view *F2, float *prev_matched, int window_size,
                                 float nn_ratio, int check_orientation, int *matches12, int *n_matches, int *matched_distance) {
    FT_REQUIRE(ctx && F1 && F2, "ft_search_for_initialization: null argument");
    FT_REQUIRE(window_size > 0, "ft_search_for_initialization: window_size must be positive");
    FT_REQUIRE(F2->Nleft == -1, "ft_search_for_initialization: F2 must be a mono / rectified frame (Nleft == -1)");
    const int N1 = F1->N, N2 = F2->N;
    FT_REQUIRE(N1 >= 0 && N1 < (1 << 24) && N2 >= 0 && N2 < (1 << 24), "ft_search_for_initialization: keypoint count out of range");
    FT_REQUIRE(N1 == 0 || (F1->keys && F1->descriptors && prev_matched && matches12), "ft_search_for_initialization: null array of F1");
    FT_REQUIRE(N2 == 0 || (F2->keys && F2->descriptors), "ft_search_for_initialization: null array of F2");
    FT_REQUIRE(F2->nlevels >= 1 && F2->nlevels <= FT_MAX_LEVELS, "ft_search_for_initialization: nlevels of F2 out of range");
    int cap1 = 0, cap2 = 0;
    for (int i = 0; i < N1; i++) {
        FT_REQUIRE(F1->keys[i].octave >= 0, "ft_search_for_initialization: negative keypoint octave");
        cap1 += F1->keys[i].octave == 0 ? 1 : 0;
    }
    for (int i = 0; i < N2; i++) {
        FT_REQUIRE(F2->keys[i].octave >= 0 && F2->keys[i].octave < F2->nlevels, "keypoint octave outside [0, nlevels)");
        cap2 += F2->keys[i].octave == 0 ? 1 : 0;
    }
    for (int i = 0; i < N1; i++) matches12[i] = -1;
    if (n_matches) *n_matches = 0;
    if (matched_distance)
        for (int i = 0; i < N2; i++) matched_distance[i] = INT_MAX;
    if (cap1 == 0 || cap2 == 0) return FT_OK;  // no row, or no candidate for any
    int rc = checkInitCaps(cap1, cap2);
    if (rc != FT_OK) return rc;
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    Arena a;
    const size_t oKeys1 = a.take(sizeof(ft_keypoint) * (size_t)N1), oDesc1 = a.take(32 * (size_t)N1);
    const size_t oKeys2 = a.take(sizeof(ft_keypoint) * (size_t)N2), oDesc2 = a.take(32 * (size_t)N2);
    const InitLayout L = layoutInit(a, N1, N2, cap1, cap2, matched_distance != nullptr);
    const size_t inputBytes = L.prev + 8 * (size_t)N1;
    const size_t oGrid = layoutGrid(a, N2);
    rc = ft_ensure_scratch(ctx, a.off, L.outEnd);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    memcpy(pin + oKeys1, F1->keys, sizeof(ft_keypoint) * (size_t)N1);
    memcpy(pin + oDesc1, F1->descriptors, 32 * (size_t)N1);
    memcpy(pin + oKeys2, F2->keys, sizeof(ft_keypoint) * (size_t)N2);
    memcpy(pin + oDesc2, F2->descriptors, 32 * (size_t)N2);
    memcpy(pin + L.prev, prev_matched, 8 * (size_t)N1);
    CallEventTimer own;
    CallScope C{ctx, ctx->stream, dev, pin, own.evt};
    C.up(0, inputBytes);
    FtInitSearch S;
    memset(&S, 0, sizeof S);
    S.F2 = devFrameConstants(F2);
    S.F2.keys = (const ft_keypoint *)(dev + oKeys2);
    S.F2.keysR = S.F2.keys;
    S.F2.desc = dev + oDesc2;
    // the grid of F2, whatever option search_grid says for the projection searches: this search walks nothing else
    C.launch(nullptr, [&] { return launchGrid(C.st, S.F2, (int *)(dev + oGrid)); });
    S.keys1 = (const ft_keypoint *)(dev + oKeys1);
    S.desc1 = dev + oDesc1;
    S.N1 = N1;
    S.window = (float)window_size;
    S.nnRatio = nn_ratio;
    S.checkOrientation = check_orientation != 0;
    S.cap1 = cap1;
    S.cap2 = cap2;
    rc = runInitSearch(C, S, L, prev_matched, matches12, n_matches, matched_distance, N2);
    if (rc != FT_OK) return rc;
    ctx->addStat("search_for_initialization.total", tAll.ms());
    ctx->addStat("search_for_initialization.launches", C.launches);
    return FT_OK;
}

int ft_tracked_frame_search_for_initialization(ft_tracked_frame *current, ft_tracked_frame *initial, float *prev_matched, int window_size,
                                               float nn_ratio, int check_orientation, int *matches12, int *n_matches) {
    FT_REQUIRE(current && initial, "ft_tracked_frame_search_for_initialization: null tracked frame");
    FT_REQUIRE(current->loaded && initial->loaded, "ft_tracked_frame_search_for_initialization: no frame loaded");
    FT_REQUIRE(current->ctx == initial->ctx, "ft_tracked_frame_search_for_initialization: the frames belong to different contexts");
    FT_REQUIRE(window_size > 0, "ft_tracked_frame_search_for_initialization: window_size must be positive");
    FT_REQUIRE(current->DF.Nleft == -1, "ft_tracked_frame_search_for_initialization: the current frame must be a mono / rectified frame (Nleft == -1)");
    FT_REQUIRE(initial->DF.Nleft == -1, "ft_tracked_frame_search_for_initialization: the initial frame must be a mono / rectified frame (Nleft == -1)");
    ft_context *ctx = current->ctx;
    const int N1 = initial->DF.N, N2 = current->DF.N;
    FT_REQUIRE(N1 == 0 || (prev_matched && matches12), "ft_tracked_frame_search_for_initialization: null array");
    for (int i = 0; i < N1; i++) matches12[i] = -1;
    if (n_matches) *n_matches = 0;
    const int cap1 = initial->level0, cap2 = current->level0;
    if (cap1 == 0 || cap2 == 0) return FT_OK;
    int rc = checkInitCaps(cap1, cap2);
    if (rc != FT_OK) return rc;
    rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    Arena a;
    const InitLayout L = layoutInit(a, N1, N2, cap1, cap2, false);
    ft_tracked_frame *tf = current;
    rc = ensureInitArena(tf, a.off, L.outEnd);
    if (rc != FT_OK) return rc;
    CallScope C{ctx, ctx->stream, tf->d_init, tf->h_init, tf->evt};
    memcpy(C.pin + L.prev, prev_matched, 8 * (size_t)N1);
    C.up(L.prev, L.prev + 8 * (size_t)N1);
    FtInitSearch S;
    memset(&S, 0, sizeof S);
    S.F2 = current->DF;
    // option search_grid = 0 when the frame was loaded: the grid for this call
    if (!S.F2.gridStart[0]) C.launch(nullptr, [&] { return launchGrid(C.st, S.F2, tf->d_grid); });
    S.keys1 = initial->DF.keys;
    S.desc1 = initial->DF.desc;
    S.N1 = N1;
    S.window = (float)window_size;
    S.nnRatio = nn_ratio;
    S.checkOrientation = check_orientation != 0;
    S.cap1 = cap1;
    S.cap2 = cap2;
    rc = runInitSearch(C, S, L, prev_matched, matches12, n_matches, nullptr, N2);
    if (rc != FT_OK) return rc;
    ctx->addStat("tracked.search_for_initialization.total", tAll.ms());
    ctx->addStat("tracked.search_for_initialization.launches", C.launches);
    return FT_OK;
}

}  // extern "C"

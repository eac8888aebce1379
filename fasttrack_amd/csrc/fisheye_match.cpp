// Host side of the brute-force Hamming calls on one frame: ft_fisheye_match and ft_fisheye_stereo replace
// KernelController::launchFisheyeStereoMatchKernel (reference include/Kernels/KernelController.h:38), ft_descriptor_distance is
// ORBmatcher::DescriptorDistance over a list of pairs.  One-shot calls on the call skeleton of search_host.h (Arena,
// CallScope); all compute is in kernels_fisheye.hip.  The same matching for every frame of a tracked batch: tracked_batch.cpp.
#include <algorithm>
#include <cstring>

#include "search_host.h"

extern "C" {

int ft_fisheye_match(ft_context *ctx, const uint8_t *descL, int nL, const uint8_t *descR, int nR, int *matches,
                     int *best, int *second) {
    FT_REQUIRE(ctx && matches, "ft_fisheye_match: null argument");
    FT_REQUIRE(nL >= 0 && nR >= 0 && nR < (1 << 20), "ft_fisheye_match: count out of range");
    FT_REQUIRE((nL == 0 || descL) && (nR == 0 || descR), "ft_fisheye_match: null descriptors");
    if (nL == 0) return FT_OK;
    int rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    // the arena: descL | descR || matches, best, second
    Arena a;
    const size_t oL = a.take((size_t)32 * nL), oR = a.take((size_t)32 * std::max(nR, 1));
    const size_t oOut = a.take(sizeof(int) * 3 * (size_t)nL);
    rc = ft_ensure_scratch(ctx, a.off, a.off);
    if (rc != FT_OK) return rc;
    uint8_t *dev = (uint8_t *)ctx->scratchDev, *pin = (uint8_t *)ctx->scratchPin;
    int *dOut = (int *)(dev + oOut), *hOut = (int *)(pin + oOut);
    hipStream_t st = ctx->stream;
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    // pageable descriptors go up through the pinned mirror (one host memcpy each) instead of being staged and waited for by
    // the runtime copy by copy; descriptors the caller keeps in pinned memory are read where they are
    auto up = [&](size_t off, const uint8_t *src, size_t bytes) {
        if (ft_is_pinned_host_range(src, bytes)) return C.upFrom(off, src, bytes);
        memcpy(pin + off, src, bytes);
        C.up(off, off + bytes);
    };
    up(oL, descL, (size_t)32 * nL);
    if (nR > 0) up(oR, descR, (size_t)32 * nR);
    C.launch(nullptr, [&] { return ft_launch_fisheye(st, dev + oL, nL, dev + oR, nR, dOut, dOut + nL, dOut + 2 * (size_t)nL); });
    rc = C.down(oOut, a.off);
    if (rc != FT_OK) return rc;
    memcpy(matches, hOut, sizeof(int) * nL);
    if (best) memcpy(best, hOut + nL, sizeof(int) * nL);
    if (second) memcpy(second, hOut + 2 * (size_t)nL, sizeof(int) * nL);
    return FT_OK;
}

int ft_fisheye_stereo(ft_context *ctx, const ft_fisheye_rig *rig, const uint8_t *descL, const ft_keypoint *keysL, int nL,
                      const uint8_t *descR, const ft_keypoint *keysR, int nR, const float *level_sigma2, int nlevels,
                      int *matches, float *depth, float *p3d, int *n_matches) {
    FT_REQUIRE(ctx && rig && matches && depth && p3d && level_sigma2, "ft_fisheye_stereo: null argument");
    FT_REQUIRE(nL >= 0 && nR >= 0 && nR < (1 << 20), "ft_fisheye_stereo: count out of range");
    FT_REQUIRE(nlevels >= 1 && nlevels <= FT_MAX_LEVELS, "ft_fisheye_stereo: nlevels out of range");
    FT_REQUIRE((nL == 0 || (descL && keysL)) && (nR == 0 || (descR && keysR)), "ft_fisheye_stereo: null keypoints / descriptors");
    for (int i = 0; i < nL; i++) FT_REQUIRE(keysL[i].octave >= 0 && keysL[i].octave < nlevels, "ft_fisheye_stereo: left octave out of range");
    for (int i = 0; i < nR; i++) FT_REQUIRE(keysR[i].octave >= 0 && keysR[i].octave < nlevels, "ft_fisheye_stereo: right octave out of range");
    if (n_matches) *n_matches = 0;
    if (nL == 0) return FT_OK;
    int rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    FtFisheyeRig G;
    memset(&G, 0, sizeof G);
    memcpy(G.cam1, rig->cam1, sizeof G.cam1);
    memcpy(G.cam2, rig->cam2, sizeof G.cam2);
    G.precision = rig->precision;
    memcpy(G.Rlr, rig->Rlr, sizeof G.Rlr);
    memcpy(G.tlr, rig->tlr, sizeof G.tlr);
    for (int i = 0; i < nlevels; i++) G.sigma2[i] = level_sigma2[i];
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    // the arena: descL | descR | keysL | keysR | count (0) || matches, best, second | depth | p3d
    Arena a;
    const size_t nRa = (size_t)std::max(nR, 1);
    const size_t oDL = a.take((size_t)32 * nL), oDR = a.take(32 * nRa), oKL = a.take(sizeof(ft_keypoint) * nL),
                 oKR = a.take(sizeof(ft_keypoint) * nRa), oCount = a.take(sizeof(int));
    const size_t inputEnd = a.off;
    const size_t oM = a.take(sizeof(int) * 3 * (size_t)nL), oOut = a.take(sizeof(float) * 4 * (size_t)nL);
    rc = ft_ensure_scratch(ctx, a.off, a.off);
    if (rc != FT_OK) return rc;
    uint8_t *dev = (uint8_t *)ctx->scratchDev, *pin = (uint8_t *)ctx->scratchPin;
    int *dM = (int *)(dev + oM), *dCount = (int *)(dev + oCount);
    float *dOut = (float *)(dev + oOut);
    hipStream_t st = ctx->stream;
    memcpy(pin + oDL, descL, (size_t)32 * nL);
    memcpy(pin + oKL, keysL, sizeof(ft_keypoint) * nL);
    if (nR > 0) {
        memcpy(pin + oDR, descR, (size_t)32 * nR);
        memcpy(pin + oKR, keysR, sizeof(ft_keypoint) * nR);
    }
    memset(pin + oCount, 0, sizeof(int));
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, inputEnd);
    C.launch(nullptr, [&] { return ft_launch_fisheye(st, dev + oDL, nL, dev + oDR, nR, dM, dM + nL, dM + 2 * (size_t)nL); });
    C.launch(nullptr, [&] {
        return ft_launch_fisheye_triangulate(st, G, (const ft_keypoint *)(dev + oKL), nL, (const ft_keypoint *)(dev + oKR), dM, dOut,
                                             dOut + nL, dCount);
    });
    rc = C.down(oCount, a.off);
    if (rc != FT_OK) return rc;
    const int *hM = (const int *)(pin + oM);
    const float *hOut = (const float *)(pin + oOut);
    memcpy(matches, hM, sizeof(int) * nL);
    memcpy(depth, hOut, sizeof(float) * nL);
    memcpy(p3d, hOut + nL, sizeof(float) * 3 * (size_t)nL);
    if (n_matches) *n_matches = *(const int *)(pin + oCount);
    return FT_OK;
}

int ft_descriptor_distance(ft_context *ctx, const uint8_t *a, const uint8_t *b, int n, int *dist) {
    FT_REQUIRE(ctx && n >= 0 && (n == 0 || (a && b && dist)), "ft_descriptor_distance: bad argument");
    if (n == 0) return FT_OK;
    int rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    Arena ar;
    const size_t oA = ar.take((size_t)32 * n), oB = ar.take((size_t)32 * n), oD = ar.take(sizeof(int) * (size_t)n);
    rc = ft_ensure_scratch(ctx, ar.off, ar.off);
    if (rc != FT_OK) return rc;
    uint8_t *dev = (uint8_t *)ctx->scratchDev, *pin = (uint8_t *)ctx->scratchPin;
    hipStream_t st = ctx->stream;
    memcpy(pin + oA, a, (size_t)32 * n);
    memcpy(pin + oB, b, (size_t)32 * n);
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, oD);
    C.launch(nullptr, [&] { return ft_launch_hamming_pairs(st, dev + oA, dev + oB, n, (int *)(dev + oD)); });
    rc = C.down(oD, oD + sizeof(int) * (size_t)n);
    if (rc != FT_OK) return rc;
    memcpy(dist, pin + oD, sizeof(int) * (size_t)n);
    return FT_OK;
}

}  // extern "C"

// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:329-403) for every map point of a call: the loops of
// LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:312-323), SearchInNeighbors (:806-816) and CreateNewMapPoints (:704) call it
// for points that do not depend on each other.  The host checks the offsets, bins the points by list length into the job lists of
// kernels_distinct.hip and enqueues: one block up (offsets, descriptors, jobs, the -1 of best_index / best_median), at most three
// launches - one per length class that occurs - and the results down; it waits once.  Nothing of that sequence depends on the
// number of points.
#include "search_host.h"

namespace {

const char *const FN = "ft_distinctive_descriptors";

// the length class of a non-empty list: 0 N <= 8, 1 N <= 16 (k_distinct_short), 2 N <= 64 (k_distinct_wave), 3 (k_distinct_block)
inline int lengthClass(int n) { return n <= 8 ? 0 : n <= 16 ? 1 : n <= 64 ? 2 : 3; }

}  // namespace

extern "C" {

int ft_distinctive_descriptors(ft_context *ctx, int n_points, const int *obs_offsets, const uint8_t *descriptors, int *best_index,
                               int *best_median, uint8_t *out_descriptors) {
    FT_REQUIRE(ctx && obs_offsets && best_index, std::string(FN) + ": null argument");
    FT_REQUIRE(n_points >= 0, std::string(FN) + ": n_points < 0");
    FT_REQUIRE(obs_offsets[0] == 0, std::string(FN) + ": obs_offsets[0] != 0");
    // the arena: offsets | descriptors | jobs | best_index (-1) | best_median (-1) || out_descriptors; what a point adds to it
    // besides its descriptors: an offset, a job, two results, 32 bytes
    const size_t perPoint = 4 + 4 + 4 + 4 + 32, slack = 6 * 64 + 4;
    int count[4] = {0, 0, 0, 0};
    for (int p = 0; p < n_points; p++) {
        const long long n = (long long)obs_offsets[p + 1] - obs_offsets[p];
        FT_REQUIRE(n >= 0, std::string(FN) + ": obs_offsets decreases at point " + std::to_string(p));
        if (n > FT_DISTINCT_MAX_OBSERVATIONS) {
            ft_set_error(std::string(FN) + ": point " + std::to_string(p) + " has " + std::to_string(n) + " descriptors, more than the " +
                         std::to_string(FT_DISTINCT_MAX_OBSERVATIONS) + " a list may hold");
            return FT_ERR_CAPACITY;
        }
        if (32 * (size_t)obs_offsets[p + 1] + perPoint * ((size_t)p + 1) + slack >= 0xffffffffull) {
            ft_set_error(std::string(FN) + ": the points of one call exceed 4 GB at point " + std::to_string(p));
            return FT_ERR_CAPACITY;
        }
        if (n) count[lengthClass((int)n)]++;
    }
    const int total = obs_offsets[n_points];
    FT_REQUIRE(total == 0 || descriptors, std::string(FN) + ": null descriptors");
    const int nJobs = count[0] + count[1] + count[2] + count[3];
    if (nJobs == 0) {  // n_points == 0 or every list empty (:365): nothing to compute, nothing of out_descriptors is written
        for (int p = 0; p < n_points; p++) best_index[p] = -1;
        if (best_median)
            for (int p = 0; p < n_points; p++) best_median[p] = -1;
        return FT_OK;
    }
    int rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    const size_t np = (size_t)n_points;
    Arena a;
    const size_t oOffsets = a.take(4 * (np + 1));
    const size_t oDesc = a.take(32 * (size_t)total);
    const size_t oJobs = a.take(4 * (size_t)nJobs);
    const size_t oIdx = a.take(4 * np);
    const size_t oMed = a.take(4 * np);
    const size_t inputEnd = a.off;
    const size_t oOut = a.take(32 * np);
    if (a.off >= 0xffffffffull) {  // (the loop above has bounded it)
        ft_set_error(std::string(FN) + ": the points of one call exceed 4 GB");
        return FT_ERR_CAPACITY;
    }
    rc = ft_ensure_scratch(ctx, a.off, a.off);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    memcpy(pin + oOffsets, obs_offsets, 4 * (np + 1));
    memcpy(pin + oDesc, descriptors, 32 * (size_t)total);
    // the job lists, one behind the other, each in point order
    int next[4] = {0, count[0], count[0] + count[1], count[0] + count[1] + count[2]};
    int *jobs = (int *)(pin + oJobs);
    for (int p = 0; p < n_points; p++) {
        const int n = obs_offsets[p + 1] - obs_offsets[p];
        if (n) jobs[next[lengthClass(n)]++] = p;
    }
    memset(pin + oIdx, 0xff, inputEnd - oIdx);  // what no kernel writes is -1: the points with an empty list
    FtDistinctCall T;
    memset(&T, 0, sizeof T);
    T.arena = dev;
    T.offsets = (unsigned)oOffsets;
    T.desc = (unsigned)oDesc;
    T.jobs = (unsigned)oJobs;
    T.bestIdx = (unsigned)oIdx;
    T.bestMedian = (unsigned)oMed;
    T.outDesc = (unsigned)oOut;
    T.n8 = count[0];
    T.n16 = count[1];
    T.nWave = count[2];
    T.nBlock = count[3];
    hipStream_t st = ctx->stream;
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, inputEnd);  // one copy: the block is contiguous
    if (T.n8 + T.n16) C.launch("kernel.distinct_short", [&] { return ft_launch_distinct_short(st, T); });
    if (T.nWave) C.launch("kernel.distinct_wave", [&] { return ft_launch_distinct_wave(st, T); });
    if (T.nBlock) C.launch("kernel.distinct_block", [&] { return ft_launch_distinct_block(st, T); });
    rc = C.down(oIdx, a.off);
    if (rc != FT_OK) return rc;
    memcpy(best_index, pin + oIdx, 4 * np);
    if (best_median) memcpy(best_median, pin + oMed, 4 * np);
    if (out_descriptors)  // the 32 bytes of a point with an empty list stay as the caller passed them (:365)
        for (int k = 0; k < nJobs; k++) memcpy(out_descriptors + 32 * (size_t)jobs[k], pin + oOut + 32 * (size_t)jobs[k], 32);
    ctx->addStat("distinctive_descriptors.total", tAll.ms());
    ctx->addStat("distinctive_descriptors.launches", C.launches);
    return FT_OK;
}

}  // extern "C"

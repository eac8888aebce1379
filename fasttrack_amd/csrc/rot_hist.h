// The rotation-consistency filter of the matchers on the host: the rotation bin of a match (src/ORBmatcher.cc:1880-1896,
// 489-497) and ComputeThreeMaxima (:2210-2251) on the bins' sizes - the order inside a bin does not matter to it.  Host twin of
// init_bin / three_maxima_keep (ft_search.h), which need the device's rounding intrinsics.  Plain C++, no HIP (tests/cpp/test_rot_hist.cpp).
#pragma once
#include <cmath>
#include <utility>
#include <vector>

#ifndef FT_HISTO_LENGTH
#define FT_HISTO_LENGTH 30  // (ft_internal.h)
#endif

// float arithmetic, round() half away from zero; a bin outside [0, FT_HISTO_LENGTH) is one the reference asserts against
inline int rotBin(float angle1, float angle2) {
    float rot = angle1 - angle2;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)std::round(rot * (1.0f / FT_HISTO_LENGTH));
    if (bin == FT_HISTO_LENGTH) bin = 0;
    return bin;
}

// bit b of the result = bin b is kept
inline int threeMaximaKeep(const int *sizes) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int b = 0; b < FT_HISTO_LENGTH; b++) {
        const int sz = sizes[b];
        if (sz > max1) {
            max3 = max2; max2 = max1; max1 = sz;
            ind3 = ind2; ind2 = ind1; ind1 = b;
        } else if (sz > max2) {
            max3 = max2; max2 = sz;
            ind3 = ind2; ind2 = b;
        } else if (sz > max3) {
            max3 = sz; ind3 = b;
        }
    }
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
    return (ind1 >= 0 ? 1 << ind1 : 0) | (ind2 >= 0 ? 1 << ind2 : 0) | (ind3 >= 0 ? 1 << ind3 : 0);
}

// The histogram of a search: add() files a match (whatever `id` names it) under its bin, forDropped() visits the matches of
// the bins ComputeThreeMaxima does not keep.
struct RotHist {
    int sizes[FT_HISTO_LENGTH] = {};
    std::vector<std::pair<int, int>> filed;  // (bin, id)
    void add(float angle1, float angle2, int id) {
        const int bin = rotBin(angle1, angle2);
        if (bin >= 0 && bin < FT_HISTO_LENGTH) sizes[bin]++, filed.emplace_back(bin, id);  // (the reference asserts)
    }
    template <typename Fn>
    void forDropped(Fn drop) const {
        const int keep = threeMaximaKeep(sizes);
        for (const auto &m : filed)
            if (!((keep >> m.first) & 1)) drop(m.second);
    }
};

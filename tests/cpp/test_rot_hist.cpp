// rotBin / threeMaximaKeep / RotHist of rot_hist.h (the host's rotation-consistency filter) against a restatement of the
// reference's ComputeThreeMaxima (src/ORBmatcher.cc:2210-2251) on std::vector bins, as its callers use it (:489-521).
#include <cmath>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "../../fasttrack_amd/csrc/rot_hist.h"

static const int HISTO_LENGTH = 30;

// ComputeThreeMaxima, statement by statement
static void ComputeThreeMaxima(std::vector<int> *histo, const int L, int &ind1, int &ind2, int &ind3) {
    int max1 = 0;
    int max2 = 0;
    int max3 = 0;
    for (int i = 0; i < L; i++) {
        const int s = histo[i].size();
        if (s > max1) {
            max3 = max2;
            max2 = max1;
            max1 = s;
            ind3 = ind2;
            ind2 = ind1;
            ind1 = i;
        } else if (s > max2) {
            max3 = max2;
            max2 = s;
            ind3 = ind2;
            ind2 = i;
        } else if (s > max3) {
            max3 = s;
            ind3 = i;
        }
    }
    if (max2 < 0.1f * (float)max1) {
        ind2 = -1;
        ind3 = -1;
    } else if (max3 < 0.1f * (float)max1) {
        ind3 = -1;
    }
}

// the bins the caller's loop (:505-518) leaves alone, as a bitmask
static int referenceKeep(const int *sizes) {
    std::vector<int> rotHist[HISTO_LENGTH];
    for (int b = 0; b < HISTO_LENGTH; b++) rotHist[b].assign((size_t)sizes[b], 0);
    int ind1 = -1, ind2 = -1, ind3 = -1;
    ComputeThreeMaxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3);
    int keep = 0;
    for (int i = 0; i < HISTO_LENGTH; i++)
        if (i == ind1 || i == ind2 || i == ind3) keep |= 1 << i;
    return keep;
}

static int bad = 0;
static void expect(bool ok, const char *what) {
    if (!ok) {
        bad++;
        printf("FAILED: %s\n", what);
    }
}

// sizes from (bin, size) pairs
struct Hist {
    int s[HISTO_LENGTH] = {};
    Hist(std::initializer_list<std::pair<int, int>> l) {
        for (auto &p : l) s[p.first] = p.second;
    }
};
static int bits(std::initializer_list<int> l) {
    int k = 0;
    for (int b : l) k |= 1 << b;
    return k;
}
static void hand(const Hist &h, int want, const char *what) {
    expect(threeMaximaKeep(h.s) == want, what);
    expect(referenceKeep(h.s) == want, what);
}

int main() {
    static_assert(FT_HISTO_LENGTH == HISTO_LENGTH, "histogram length");
    // ---- seeded histograms ----
    std::mt19937 rng(20240611);
    int checked = 0;
    for (int trial = 0; trial < 6000; trial++) {
        int sizes[HISTO_LENGTH];
        const int top = trial % 4 == 0 ? 3 : 13;  // small ranges: many ties
        for (int b = 0; b < HISTO_LENGTH; b++) sizes[b] = (int)(rng() % top);
        if (trial % 5 == 0)
            for (int b = 0; b < HISTO_LENGTH; b++)
                if (rng() % 3) sizes[b] = 0;  // sparse
        if (threeMaximaKeep(sizes) != referenceKeep(sizes)) bad++;
        // RotHist drops exactly the matches of the other bins
        RotHist h;
        std::set<int> wantDropped, dropped;
        const int keep = referenceKeep(sizes);
        int id = 0;
        for (int b = 0; b < HISTO_LENGTH; b++)
            for (int k = 0; k < sizes[b]; k++, id++) {
                h.add(30.0f * (float)b, 0.0f, id);  // bin b
                if (!((keep >> b) & 1)) wantDropped.insert(id);
            }
        h.forDropped([&](int i) { dropped.insert(i); });
        if (dropped != wantDropped) bad++;
        checked++;
    }
    // ---- hand cases ----
    hand(Hist{}, 0, "all zero keeps nothing");
    hand(Hist{{7, 4}}, bits({7}), "one non-empty bin");
    hand(Hist{{2, 5}, {9, 5}, {20, 5}, {25, 4}}, bits({2, 9, 20}), "the three largest equal");
    hand(Hist{{0, 10}, {1, 1}}, bits({0, 1}), "max1 10, max2 1: 1 < 1.0 is false, bin 2 kept");
    hand(Hist{{0, 11}, {1, 1}}, bits({0}), "max1 11, max2 1: bin 2 dropped");
    hand(Hist{{0, 10}, {1, 5}, {2, 1}}, bits({0, 1, 2}), "max1 10, max3 1: bin 3 kept");
    hand(Hist{{0, 11}, {1, 5}, {2, 1}}, bits({0, 1}), "max1 11, max3 1: bin 3 dropped");
    hand(Hist{{4, 9}, {10, 6}, {11, 6}, {12, 6}}, bits({4, 10, 11}), "tie between second and third: the earlier bins win");
    hand(Hist{{29, 3}, {3, 7}, {0, 3}}, bits({3, 0, 29}), "tie for third with nothing behind it");
    // ---- bins ----
    expect(rotBin(-0.0f, 0.0f) == 0 && rotBin(0.0f, 0.0f) == 0, "difference -0.0 / 0.0: bin 0");
    expect(rotBin(359.99f, 0.0f) == 12, "359.99: bin 12");
    expect(rotBin(345.0f, 0.0f) == 12, "345.0: 11.5 rounds half away to bin 12");
    expect(rotBin(15.0f, 0.0f) == 1, "15.0: 0.5 rounds half away to bin 1");
    expect(rotBin(0.0f, 15.0f) == 12, "-15.0 + 360 = 345.0: bin 12");
    expect(rotBin(0.0f, 1e-6f) == 12, "a negative difference that rounds to 360.0: bin 12");
    expect((int)std::round(885.0f * (1.0f / 30)) == 30 && rotBin(885.0f, 0.0f) == 0, "a difference that rounds to 30 wraps to 0");
    {   // a bin outside the histogram is not filed (the reference asserts)
        RotHist h;
        h.add(2000.0f, 0.0f, 1);
        expect(h.filed.empty(), "bins outside [0, 30) are not filed");
    }
    printf("histograms %d mismatches %d\n", checked, bad);
    return bad ? 1 : 0;
}

// fv_host.h, the host's one FeatureVector helper: checkFv against every rejection it names, layoutFv / stageFv against offsets and
// bytes written out by hand, guard bytes around everything staged.  Plain C++ (no HIP, nothing of the library is linked).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../fasttrack_amd/csrc/fv_host.h"

static int bad = 0, checks = 0;
static void expect(bool ok, const std::string &what) {
    checks++;
    if (!ok) {
        bad++;
        printf("FAILED: %s\n", what.c_str());
    }
}

// what the public structs look like to fvOf: ft_bow_side and ft_triang_keyframe have these fields among others
struct Side {
    int n, n_nodes;
    const unsigned *fv_nodes;
    const int *fv_offsets;
    const unsigned *fv_features;
};

// a FeatureVector held in vectors, with a copy to prove that a check writes nothing
struct Fv {
    int n;
    std::vector<unsigned> nodes;
    std::vector<int> offsets;
    std::vector<unsigned> feats;
    FvView view() const {
        const Side s{n, (int)nodes.size(), nodes.data(), offsets.data(), feats.empty() ? nullptr : feats.data()};
        return fvOf(s);
    }
};

static void rejects(const Fv &f, bool unique, const char *want, const char *what) {
    const Fv before = f;
    const char *got = checkFv(f.view(), unique);
    if (want) expect(got && std::string(got) == want, std::string(what) + ": " + (got ? got : "(accepted)"));
    else expect(!got, std::string(what) + ": " + (got ? got : ""));
    expect(before.nodes == f.nodes && before.offsets == f.offsets && before.feats == f.feats, std::string(what) + ": inputs untouched");
}

static const uint8_t GUARD = 0xA5;

// stages `f` at the arena's current end into a guarded mirror; want: the bytes expected at each of the three offsets
struct Expected {
    size_t nodes, offsets, feats, end;
    std::vector<unsigned> nodesWords;
    std::vector<int> offsetWords;
    std::vector<unsigned> featWords;
};
static void stages(Arena &a, const Fv &f, const Expected &E, const char *what) {
    const std::string w = what;
    const FvView v = f.view();
    const FvLayout L = layoutFv(a, v);
    expect(L.nodes == E.nodes && L.offsets == E.offsets && L.feats == E.feats, w + ": offsets");
    expect(L.total == (int)E.featWords.size(), w + ": total");
    expect(a.off == E.end && a.off % 64 == 0, w + ": the arena ends on a 64-byte boundary");
    std::vector<uint8_t> pin(a.off + 64, GUARD);  // (64 guard bytes behind the arena as well)
    const FtFv D = stageFv(v, L, pin.data());
    expect(D.n == f.n && D.nNodes == (int)f.nodes.size() && D.nodes == E.nodes && D.offsets == E.offsets && D.feats == E.feats, w + ": record");
    std::vector<uint8_t> want(pin.size(), GUARD);
    if (!E.nodesWords.empty()) memcpy(want.data() + E.nodes, E.nodesWords.data(), 4 * E.nodesWords.size());
    memcpy(want.data() + E.offsets, E.offsetWords.data(), 4 * E.offsetWords.size());
    if (!E.featWords.empty()) memcpy(want.data() + E.feats, E.featWords.data(), 4 * E.featWords.size());
    expect(pin == want, w + ": staged bytes, and no byte outside them");
}

int main() {
    // ---- validation ----
    const Fv good{6, {1, 5, 8}, {0, 2, 2, 5}, {4, 0, 1, 3, 5}};
    rejects(good, false, nullptr, "a 3-node vector");
    rejects(good, true, nullptr, "a 3-node vector, unique");
    rejects(Fv{0, {}, {0}, {}}, true, nullptr, "an empty vector");
    {
        const Side s{4, 0, nullptr, nullptr, nullptr};
        expect(!checkFv(fvOf(s), true), "no nodes: null arrays are never read");
        const Side t{4, 2, nullptr, nullptr, nullptr};
        const char *got = checkFv(fvOf(t), false);
        expect(got && !strcmp(got, "null feature vector"), "null nodes / offsets with n_nodes > 0");
        const unsigned nodes[2] = {1, 2};
        const int offsets[3] = {0, 1, 2};
        const Side u{4, 2, nodes, offsets, nullptr};
        got = checkFv(fvOf(u), false);
        expect(got && !strcmp(got, "null fv_features"), "null fv_features with entries");
    }
    rejects(Fv{6, {1, 5, 8}, {1, 2, 2, 5}, {4, 0, 1, 3, 5}}, false, "fv_offsets[0] != 0", "fv_offsets[0] != 0");
    rejects(Fv{6, {1, 5, 8}, {0, 3, 2, 5}, {4, 0, 1, 3, 5}}, false, "fv_offsets not ascending", "offsets descending");
    rejects(Fv{6, {1, 5, 5}, {0, 2, 2, 5}, {4, 0, 1, 3, 5}}, false, "fv_nodes not strictly ascending", "nodes equal");
    rejects(Fv{6, {1, 8, 5}, {0, 2, 2, 5}, {4, 0, 1, 3, 5}}, false, "fv_nodes not strictly ascending", "nodes descending");
    rejects(Fv{4, {1, 5, 8}, {0, 2, 2, 5}, {3, 0, 1, 2, 3}}, false, "more feature-vector entries than features", "more entries than features");
    rejects(Fv{6, {1, 5, 8}, {0, 2, 2, 5}, {4, 0, 6, 3, 5}}, false, "feature index out of range", "index n");
    rejects(Fv{6, {1, 5, 8}, {0, 2, 2, 5}, {4, 0, 6, 3, 5}}, true, "feature index out of range", "index n, unique");
    rejects(Fv{6, {1, 5, 8}, {0, 2, 2, 5}, {4, 0, 1, 4, 5}}, true, "a feature is listed twice", "a duplicate, unique on");
    rejects(Fv{6, {1, 5, 8}, {0, 2, 2, 5}, {4, 0, 1, 4, 5}}, false, nullptr, "a duplicate, unique off");
    rejects(Fv{6, {1, 5, 8}, {0, 2, 2, 5}, {4, 0, 1, 3, 5}}, true, nullptr, "index n - 1 and 0 are in range");

    // ---- layout and staging: every block starts on a 64-byte boundary, an empty block still has room for one word ----
    {   // an empty side at the start of an arena: only the one offset, 0, is written
        Arena a;
        stages(a, Fv{0, {}, {0}, {}}, Expected{0, 64, 128, 192, {}, {0}, {}}, "empty side");
    }
    {   // behind 10 bytes of something else: nodes at 64.  Two nodes, no entry: 8 bytes of nodes, 12 of offsets, nothing of feats
        Arena a;
        expect(a.take(10) == 0 && a.off == 64, "take rounds up to 64");
        stages(a, Fv{5, {3, 9}, {0, 0, 0}, {}}, Expected{64, 128, 192, 256, {3, 9}, {0, 0, 0}, {}}, "nodes without entries");
    }
    {   // one node holding feature n - 1, behind a block that ends on a boundary already
        Arena a;
        expect(a.take(128) == 0 && a.off == 128, "a full block is not padded");
        stages(a, Fv{7, {42}, {0, 1}, {6}}, Expected{128, 192, 256, 320, {42}, {0, 1}, {6}}, "one node, feature n - 1");
    }
    {   // three nodes, the middle one empty
        Arena a;
        stages(a, good, Expected{0, 64, 128, 192, {1, 5, 8}, {0, 2, 2, 5}, {4, 0, 1, 3, 5}}, "three nodes");
    }
    {   // 17 nodes: 68 bytes of nodes and 72 of offsets take two 64-byte units each
        Fv f{40, {}, {0}, {}};
        Expected E{0, 128, 256, 384, {}, {0}, {}};
        for (int j = 0; j < 17; j++) {
            f.nodes.push_back(100 + 3 * j);
            f.feats.push_back(39 - j);
            f.offsets.push_back(j + 1);
        }
        E.nodesWords = f.nodes;
        E.offsetWords = f.offsets;
        E.featWords = f.feats;
        rejects(f, true, nullptr, "17 nodes");
        Arena a;
        stages(a, f, E, "17 nodes");
    }
    printf("checks %d failed %d\n", checks, bad);
    return bad ? 1 : 0;
}

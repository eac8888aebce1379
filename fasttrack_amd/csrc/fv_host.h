// The FeatureVector of a keyframe or frame on the host - a DBoW2 std::map<NodeId, std::vector<unsigned>> in the CSR form of
// ft_bow_transform (fv_nodes ascending, the features of node j = fv_features[fv_offsets[j] .. fv_offsets[j + 1])) - as every
// matcher that walks common nodes takes it (ft_bow_side, ft_triang_keyframe): its validation, its place in a call's arena and its
// staging into the arena's pinned mirror, once.  Plain C++, no HIP (tests/cpp/test_fv_host.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// the byte offsets of a call's arena: every block starts on a 64-byte boundary
struct Arena {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off = (off + bytes + 63) & ~(size_t)63;
        return o;
    }
};

struct FvView {
    int n, n_nodes;  // features of the side, FeatureVector entries
    const unsigned *fv_nodes;
    const int *fv_offsets;
    const unsigned *fv_features;
};
// of an ft_bow_side, or of the flat fields of an ft_triang_keyframe
template <class Side>
inline FvView fvOf(const Side &s) {
    return FvView{s.n, s.n_nodes, s.fv_nodes, s.fv_offsets, s.fv_features};
}
inline int fvTotal(const FvView &v) { return v.n_nodes > 0 ? v.fv_offsets[v.n_nodes] : 0; }

// What is wrong with the FeatureVector of a side whose counts are in range (0 <= n, 0 <= n_nodes), or null.  unique: a feature
// may be listed once only - what makes the nodes of a side independent units of work for the matchers that rely on it.
inline const char *checkFv(const FvView &v, bool unique) {
    if (v.n_nodes == 0) return nullptr;
    if (!v.fv_nodes || !v.fv_offsets) return "null feature vector";
    if (v.fv_offsets[0] != 0) return "fv_offsets[0] != 0";
    for (int j = 0; j < v.n_nodes; j++) {
        if (v.fv_offsets[j + 1] < v.fv_offsets[j]) return "fv_offsets not ascending";
        if (j > 0 && v.fv_nodes[j] <= v.fv_nodes[j - 1]) return "fv_nodes not strictly ascending";
    }
    const int total = v.fv_offsets[v.n_nodes];
    if (total > v.n) return "more feature-vector entries than features";
    if (total > 0 && !v.fv_features) return "null fv_features";
    for (int e = 0; e < total; e++)
        if (v.fv_features[e] >= (unsigned)v.n) return "feature index out of range";
    if (unique) {
        std::vector<uint8_t> seen((size_t)v.n, 0);
        for (int e = 0; e < total; e++) {
            if (seen[v.fv_features[e]]) return "a feature is listed twice";  // a FeatureVector holds a feature under one node
            seen[v.fv_features[e]] = 1;
        }
    }
    return nullptr;
}

// the CSR part of a side in the arena of a call: byte offsets of nodes | offsets | feats (no block is empty, so no two share an offset)
struct FvLayout {
    size_t nodes, offsets, feats;
    int total;  // FeatureVector entries
};
// what a kernel gets of it (a record of the call's job table: the byte offsets fit 32 bits, the callers refuse arenas of 4 GB)
struct FtFv {
    int n, nNodes;                   // features, FeatureVector entries
    unsigned nodes, offsets, feats;  // unsigned[nNodes] ascending, int[nNodes + 1], unsigned[offsets[nNodes]]
};

inline FvLayout layoutFv(Arena &a, const FvView &v) {
    FvLayout L;
    const size_t nn = (size_t)v.n_nodes;
    L.total = fvTotal(v);
    L.nodes = a.take(4 * std::max(nn, (size_t)1));
    L.offsets = a.take(4 * (nn + 1));
    L.feats = a.take(4 * (size_t)std::max(L.total, 1));
    return L;
}

// pin: the arena's pinned mirror; an empty vector leaves its one offset, 0
inline FtFv stageFv(const FvView &v, const FvLayout &L, uint8_t *pin) {
    const size_t nn = (size_t)v.n_nodes;
    if (nn) {
        memcpy(pin + L.nodes, v.fv_nodes, 4 * nn);
        memcpy(pin + L.offsets, v.fv_offsets, 4 * (nn + 1));
        if (L.total) memcpy(pin + L.feats, v.fv_features, 4 * (size_t)L.total);
    } else {
        memset(pin + L.offsets, 0, 4);
    }
    return FtFv{v.n, v.n_nodes, (unsigned)L.nodes, (unsigned)L.offsets, (unsigned)L.feats};
}

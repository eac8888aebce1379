// What the entry points over ft_triang_keyframe share (triang_search.cpp: ft_search_for_triangulation; newpoints.cpp:
// ft_triangulate_new_points, ft_search_and_triangulate): the checks of a keyframe, its place in the arena and its staging, and the
// block of a call - keyframe 1 | its record | nodeOf | neighbour sides | jobs - that goes up in one copy.  `search` = the call runs
// the matcher: without it the descriptors, the FeatureVector and has_point of a keyframe are neither read nor given room.
#pragma once
#include <string>
#include <vector>

#include "search_host.h"

struct TriangSideLayout {
    size_t keys, desc, hasPoint, uright, sf, sigma2;
    FvLayout fv;
};

inline int checkTriangSide(const ft_triang_keyframe *s, const std::string &w, bool search = true) {
    FT_REQUIRE(s->n >= 0 && s->n < (1 << 20) && (!search || s->n_nodes >= 0), w + "count out of range");
    FT_REQUIRE(s->n_left >= -1 && s->n_left <= s->n, w + "n_left out of range");
    FT_REQUIRE(s->cam_model == 0 || s->cam_model == 1, w + "unknown camera model");
    FT_REQUIRE(!(s->cam_model == 0 && s->two_cameras), w + "a pinhole keyframe with two cameras");
    FT_REQUIRE(s->scale_factors && s->level_sigma2 && s->nlevels >= 1 && s->nlevels <= FT_MAX_LEVELS, w + "scale factors / level sigmas missing");
    FT_REQUIRE(s->n == 0 || (s->keys && (!search || (s->descriptors && s->has_point))), w + "keypoints, descriptors or has_point are null");
    for (int i = 0; i < s->n; i++) FT_REQUIRE(s->keys[i].octave >= 0 && s->keys[i].octave < s->nlevels, w + "keypoint octave outside [0, nlevels)");
    if (!search) return FT_OK;
    const char *what = checkFv(fvOf(*s), true);  // a FeatureVector holds a feature under one node
    FT_REQUIRE(!what, w + what);
    return FT_OK;
}

// keyframe 1 and the neighbours of a call: every side, and that they agree in two_cameras and in the camera model
inline int checkTriangCall(const std::string &fn, const ft_triang_keyframe *kf1, int n_neighbours, const ft_triang_keyframe *kf2, bool search) {
    int rc = checkTriangSide(kf1, fn + ": keyframe 1: ", search);
    if (rc != FT_OK) return rc;
    for (int k = 0; k < n_neighbours; k++) {
        rc = checkTriangSide(kf2 + k, fn + ": neighbour " + std::to_string(k) + ": ", search);
        if (rc != FT_OK) return rc;
        // the reference reads an uninitialised R12 when only one of the two keyframes has a second camera (:1027-1039, :1135)
        FT_REQUIRE(!kf2[k].two_cameras == !kf1->two_cameras && kf2[k].cam_model == kf1->cam_model,
                   fn + ": the keyframes of a call differ in two_cameras or in the camera model");
    }
    return FT_OK;
}

inline TriangSideLayout layoutTriangSide(Arena &a, const ft_triang_keyframe *s, bool search = true) {
    TriangSideLayout L;
    memset(&L, 0, sizeof L);
    const size_t n = (size_t)std::max(s->n, 1);
    L.keys = a.take(sizeof(ft_keypoint) * n);
    if (search) {
        L.desc = a.take(32 * n);
        L.fv = layoutFv(a, fvOf(*s));
        L.hasPoint = a.take(n);
    }
    L.uright = s->uright ? a.take(4 * n) : 0;
    L.sf = a.take(4 * FT_MAX_LEVELS);
    L.sigma2 = a.take(4 * FT_MAX_LEVELS);
    return L;
}

inline FtTriangSide stageTriangSide(const ft_triang_keyframe *s, const TriangSideLayout &L, uint8_t *pin, bool search = true) {
    const size_t n = (size_t)s->n;
    if (n) {
        memcpy(pin + L.keys, s->keys, sizeof(ft_keypoint) * n);
        if (search) {
            memcpy(pin + L.desc, s->descriptors, 32 * n);
            memcpy(pin + L.hasPoint, s->has_point, n);
        }
        if (s->uright) memcpy(pin + L.uright, s->uright, 4 * n);
    }
    memcpy(pin + L.sf, s->scale_factors, 4 * (size_t)s->nlevels);
    memcpy(pin + L.sigma2, s->level_sigma2, 4 * (size_t)s->nlevels);
    FtTriangSide D;
    D.fv = search ? stageFv(fvOf(*s), L.fv, pin) : FtFv{s->n, 0, 0, 0, 0};
    D.nLeft = s->n_left;
    D.keys = (unsigned)L.keys;
    D.desc = (unsigned)L.desc;
    D.hasPoint = (unsigned)L.hasPoint;
    D.uright = s->uright ? (unsigned)L.uright : FT_TRIANG_NONE;
    D.sf = (unsigned)L.sf;
    D.sigma2 = (unsigned)L.sigma2;
    memcpy(D.cam[0], s->cam, sizeof D.cam[0]);
    memcpy(D.cam[1], s->cam2, sizeof D.cam[1]);
    return D;
}

// the input block of a call
struct TriangBlock {
    TriangSideLayout L1;
    std::vector<TriangSideLayout> L2;
    size_t oK1, oNodeOf, oJobs;
    bool search;

    void layout(Arena &a, const ft_triang_keyframe *kf1, int n_neighbours, const ft_triang_keyframe *kf2, bool withSearch) {
        search = withSearch;
        L1 = layoutTriangSide(a, kf1, search);
        oK1 = a.take(sizeof(FtTriangSide));
        oNodeOf = search ? a.take(4 * (size_t)kf1->n) : 0;
        L2.resize((size_t)n_neighbours);
        for (int k = 0; k < n_neighbours; k++) L2[k] = layoutTriangSide(a, kf2 + k, search);
        oJobs = a.take(sizeof(FtTriangJob) * (size_t)n_neighbours);
    }
    // fills the pinned block and T up to the job records' output rows (FtTriangJob::matches / bestDist), which the caller places;
    // pairs may be null without the search
    FtTriangJob *stage(const ft_triang_keyframe *kf1, int n_neighbours, const ft_triang_keyframe *kf2, const ft_triang_pair *pairs, uint8_t *pin,
                       uint8_t *dev, FtTriangCall &T) const {
        memset(&T, 0, sizeof T);
        T.arena = dev;
        T.K1 = stageTriangSide(kf1, L1, pin, search);
        memcpy(pin + oK1, &T.K1, sizeof T.K1);
        T.k1 = (unsigned)oK1;
        if (search) {
            int *nodeOf = (int *)(pin + oNodeOf);
            for (int i = 0; i < kf1->n; i++) nodeOf[i] = -1;
            for (int j = 0; j < kf1->n_nodes; j++)
                for (int e = kf1->fv_offsets[j]; e < kf1->fv_offsets[j + 1]; e++) nodeOf[kf1->fv_features[e]] = j;
        }
        T.nodeOf = (unsigned)oNodeOf;
        FtTriangJob *jobs = (FtTriangJob *)(pin + oJobs);
        for (int k = 0; k < n_neighbours; k++) {
            FtTriangJob &J = jobs[k];
            memset(&J, 0, sizeof J);
            J.K2 = stageTriangSide(kf2 + k, L2[k], pin, search);
            if (pairs) {
                memcpy(J.ep, pairs[k].ep, sizeof J.ep);
                memcpy(J.F12, pairs[k].F12, sizeof J.F12);
                memcpy(J.R12, pairs[k].R12, sizeof J.R12);
                memcpy(J.t12, pairs[k].t12, sizeof J.t12);
                J.precision = pairs[k].kb8_precision;
            }
        }
        T.jobs = (unsigned)oJobs;
        T.nNeighbours = n_neighbours;
        T.camModel = kf1->cam_model;
        T.twoCameras = kf1->two_cameras != 0;
        return jobs;
    }
};

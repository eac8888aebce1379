// HIP kernels of the two projection searches for gfx950 (wave64): the wave-per-point kernels.
//   k_search_local  ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>, th, ...)  (reference
//                   src/ORBmatcher.cc:49-225 + Frame::GetFeaturesInArea src/Frame.cc:681-747)
//   k_search_last   ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono)  (:1775-1960)
//   k_features_in_area                      Frame::GetFeaturesInArea for a batch of queries
//   k_search_*_batch, k_last_project_batch  the two searches for the frames of a batch (ft_tracked_batch), blockIdx.y = frame
// The other kernels of the searches: kernels_search_rows.hip (a point = a row of 16 lanes: the first pass and the lean later
// passes of a batch), kernels_resolve.hip (a batch's claims resolved in one launch, and the replay of its writes),
// kernels_frame.hip (what prepares and delivers a frame: grid, frustum, fills, deliveries).  What they share: search_dev.h.
//
// One wave per map point; without a grid, lanes stride over the frame's keypoints and test the 64x48-grid cell window,
// the level band and the box exactly as GetFeaturesInArea does, so no per-cell lists are needed (the
// reference's fixed 20-per-cell matrix overflows).  The scan order of the CPU loop,
// (cell x, cell y, keypoint index), is folded into a 64-bit key (distance, cx, cy, index): the two
// smallest keys of the wave are the CPU's (best, second best) including which octaves they carry.
//
// The grid (k_build_grid, kernels_frame.hip; FtDevFrame::gridStart / gridRec / gridDesc): one CSR per octave over the 64x48
// cells, its entries search records and descriptors in cell order.  A window's column of cells inside the search's level
// band is one contiguous range of entries per octave, so for_window reads the keypoints GetFeaturesInArea would return
// and little else, a few (octave, column) ranges laid end to end by a wave scan.  A frame without a grid is scanned whole.
//
// The candidate cache (FtClaims::cache; meta word and states in search_dev.h): the first pass that reaches a (point, camera)
// window files the keys of all its candidates - box, level band, uright test and Hamming distance do not change from pass
// to pass - and every later pass walks those keys against the new lock state instead of the window.  A list with more than
// FT_CACHE_CAP candidates is not cached: that window is scanned again.
//
// In-call claiming (a keypoint taken by an earlier map point with Observations() > 0 is skipped by
// later ones, ORBmatcher.cc:101-103,142) makes the CPU loop sequential.  It is reproduced exactly by a
// Jacobi iteration on that triangular dependency: every pass recomputes all points in parallel
// against the writes of the previous pass (per-keypoint writer records, search_dev.h); point i is final
// after at most i+1 passes and the iteration stops when a pass changes nothing - the unique fixed
// point is the sequential result.
#include <algorithm>

#include "search_dev.h"

namespace {

// geometric part of GetFeaturesInArea for one keypoint: grid cell (Frame::PosInGrid, :749-759) inside
// the window, level band, box test.  Returns false when the keypoint is not a candidate.
__device__ __forceinline__ bool in_area(const FtDevFrame &F, const ft_keypoint &kp, const Window &w, float x, float y,
                                        float r, int minLevel, int maxLevel, int &cx, int &cy) {
    cx = (int)roundf(__fmul_rn(__fsub_rn(kp.x, F.mnMinX), F.invW));
    cy = (int)roundf(__fmul_rn(__fsub_rn(kp.y, F.mnMinY), F.invH));
    if (cx < 0 || cx >= FT_GRID_COLS || cy < 0 || cy >= FT_GRID_ROWS) return false;  // never entered the grid
    if (cx < w.minCX || cx > w.maxCX || cy < w.minCY || cy > w.maxCY) return false;
    const bool checkLevels = (minLevel > 0) || (maxLevel >= 0);
    if (checkLevels) {
        if (kp.octave < minLevel) return false;
        if (maxLevel >= 0 && kp.octave > maxLevel) return false;
    }
    const float dx = __fsub_rn(kp.x, x), dy = __fsub_rn(kp.y, y);
    return fabsf(dx) < r && fabsf(dy) < r;
}

// Frame::GetFeaturesInArea (src/Frame.cc:681-747) for a batch of queries: one wave per query, lanes stride over the
// keypoints of the requested camera; hits are appended as (cell x, cell y, index) keys whose ascending order is the
// order of the reference's nested cell loops (the host sorts the few hits of a query).
__global__ __launch_bounds__(256) void k_features_in_area(FtDevFrame F, int nq, const float *qx, const float *qy, const float *qr,
                                                          const int *qmin, const int *qmax, const uint8_t *qright,
                                                          const int *offsets, unsigned *outKeys, int *outCount) {
    const int lane = threadIdx.x & 63, wave = wave_index();
    const int q = blockIdx.x * 4 + wave;
    if (q >= nq) return;
    const float x = qx[q], y = qy[q], r = qr[q];
    const int minLevel = qmin[q], maxLevel = qmax[q];
    const bool right = qright && qright[q];
    const int n = F.Nleft == -1 ? F.N : (right ? F.N - F.Nleft : F.Nleft);
    const ft_keypoint *keys = (F.Nleft != -1 && right) ? F.keysR : F.keys;
    const Window w = cell_window(F, x, y, r);
    int count = 0;
    if (!w.empty) {
        for (int base = 0; base < n; base += 64) {
            const int idx = base + lane;
            bool hit = false;
            int cx = 0, cy = 0;
            if (idx < n) hit = in_area(F, keys[idx], w, x, y, r, minLevel, maxLevel, cx, cy);
            const unsigned long long b = __ballot(hit);
            if (hit) {
                // first pass (offsets == null) only counts; the second writes every hit at the query's offset
                const int pos = count + __popcll(b & ((1ull << lane) - 1ull));
                if (offsets) outKeys[(size_t)offsets[q] + pos] = ((unsigned)cx << 26) | ((unsigned)cy << 20) | (unsigned)idx;
            }
            count += __popcll(b);
        }
    }
    if (lane == 0 && !offsets) outCount[q] = count;
}

// two smallest keys of the wave (k0 < k1)
__device__ __forceinline__ void wave_two_min(unsigned long long &k0, unsigned long long &k1) {
    const unsigned long long m0 = wave_min_u64(k0);
    const unsigned long long cand = (k0 == m0) ? k1 : k0;
    const unsigned long long m1 = wave_min_u64(cand);
    k0 = m0;
    k1 = m1;
}

// ---- candidate cache of the claim iteration (FtClaims::cache) ----
// One LDS counter per wave hands out the positions while a window is scanned (the candidates turn up in divergent code).
struct CacheBuild {
    unsigned long long *slot;  // null: no cache
    int *counter;              // LDS, this wave's
    bool build;                // wave-uniform: this scan files its candidates
};
__device__ __forceinline__ void cache_begin(CacheBuild &B, int lane) {
    if (B.build) {
        if (lane == 0) *B.counter = 0;
        wave_lds_sync();
    }
}
__device__ __forceinline__ void cache_append(const CacheBuild &B, unsigned long long key) {
    const int pos = atomicAdd(B.counter, 1);
    if (pos < FT_CACHE_CAP) B.slot[1 + pos] = key;
}
__device__ __forceinline__ void cache_end(const CacheBuild &B, int lane, bool anyInBox) {
    if (B.build) {
        wave_lds_sync();
        const int n = *B.counter;
        if (lane == 0)  // (head = count: not partitioned)
            B.slot[0] = (unsigned long long)(unsigned)n | ((unsigned long long)(anyInBox ? 1 : 0) << 32) |
                        ((unsigned long long)(unsigned)min(n, FT_CACHE_CAP) << 40);
    }
}
// cache_state_of (search_dev.h) of a list's meta word in memory; no list (slot == null) reads as 2
__device__ __forceinline__ int cache_state(const unsigned long long *slot, int &count, bool &anyInBox) {
    count = 0;
    anyInBox = false;
    if (!slot) return 2;
    const unsigned long long meta = slot[0];
    if (meta == KEY_NONE) return 0;
    count = (int)(unsigned)meta;
    anyInBox = ((meta >> 32) & 1ull) != 0;
    return count <= FT_CACHE_CAP ? 1 : 2;
}

// end of a point's turn in a pass: lane k files write kind k of point i - the result, the "changed" flag against the
// previous pass, and the entry in the writer table the NEXT pass will read (so a pass is one launch)
__device__ __forceinline__ void claims_file(const FtClaims &C, int *res, int i, int lane, const int r4[4]) {
    if (lane < 4) {
        const int kp = lane == 0 ? r4[0] : lane == 1 ? r4[1] : lane == 2 ? r4[2] : r4[3];
        const int s = 4 * i + lane;
        const int prev = C.firstPass ? 0 : shared_load(&C.resPrev[s]);
        if (!C.firstPass && kp != prev) atomicAnd(C.flagCur, 0);
        shared_store(&res[s], kp);
        if (kp >= 0) {
            const int e = (s << 1) | (C.obs[i] > 0 ? 1 : 0);
            int *rec = C.tabWrite + 8 * (size_t)kp;
            const int pos = atomicAdd(rec, 1) + 1;  // the record starts at -1
            if (pos < FT_TAB_ENTRIES) shared_store(rec + 1 + pos, e);
            else shared_store(&C.nextWrite[s], atomicExch(&C.headWrite[kp], e));
        }
    }
}

// ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th, ...) for map point i by one wave (src/ORBmatcher.cc:49-225):
// r = (primary left, side left, primary right, side right) keypoints it writes; raw outputs as the reference kernel's
__device__ __forceinline__ void local_point(const FtDevFrame &F, const FramePtrs &Q, const FtDevLocalPoints &P, const FtClaims &C, float th,
                                            float nnRatio, int i, int lane, int r4[4], const FtLocalRaw &raw, int *ldsCounter) {
    int primL = -1, sideL = -1, primR = -1, sideR = -1;
    int bd = 256, bd2 = 256, bl = -1, bl2 = -1, bi = -1;
    int bdr = 256, bd2r = 256, blr = -1, bl2r = -1, bir = -1;
    bool skipRight = false;
    unsigned long long q[4];
    {
        const unsigned long long *p = (const unsigned long long *)(P.desc + (size_t)i * 32);
        q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = p[3];
    }
    // Everything a pass needs of the point that does not depend on another load is requested HERE, before the first use: the
    // flags, both cache meta words and - speculatively - the first 64 cached keys of either camera.  A pass on cached
    // candidates was a chain of five dependent round trips (skip -> in view -> meta -> keys -> lock records); now it is two.
    unsigned long long *slotL = C.cache ? C.cache + (size_t)i * FT_CACHE_WORDS : nullptr;
    unsigned long long *slotR = slotL ? slotL + (FT_CACHE_CAP + 1) : nullptr;
    const bool twoCam = F.Nleft != -1;
    const uint8_t skipV = P.skip[i], inViewV = P.inView[i], inViewRV = twoCam ? P.inViewR[i] : (uint8_t)0;
    const int levelRV = twoCam ? P.levelR[i] : -1;
    const unsigned long long metaL = slotL ? slotL[0] : KEY_NONE, metaR = (slotR && twoCam) ? slotR[0] : KEY_NONE;
    const unsigned long long keyL0 = slotL ? slotL[1 + lane] : KEY_NONE, keyR0 = (slotR && twoCam) ? slotR[1 + lane] : KEY_NONE;
    if (!skipV) {
        const int nLeft = F.Nleft == -1 ? F.N : F.Nleft;
        if (inViewV) {
            unsigned long long k0 = KEY_NONE, k1 = KEY_NONE;
            CacheBuild cb;
            cb.slot = slotL;
            cb.counter = ldsCounter;
            int nCached;
            bool anyBox;
            const int cs = slotL ? cache_state_of(metaL, nCached, anyBox) : 2;
            cb.build = cs == 0;
            if (cs == 1) {
                for (int t = lane; t < nCached; t += 64) {
                    const unsigned long long key = t < 64 ? keyL0 : cb.slot[1 + t];
                    if (is_locked(C, key_idx(key), i, key_held(key))) continue;
                    two_min_insert(k0, k1, key);
                }
            } else {
                const int level = P.level[i];
                float r = ((double)P.viewCos[i] > 0.998) ? 2.5f : 4.0f;  // RadiusByViewingCos, ORBmatcher.cc:314-320
                if ((double)th != 1.0) r = __fmul_rn(r, th);
                const float rad = __fmul_rn(r, F.sf[level]);
                const float x = P.projX[i], y = P.projY[i];
                const Window w = cell_window(F, x, y, rad);
                cache_begin(cb, lane);
                if (!w.empty) {
                    const float pxr = (F.Nleft == -1 && Q.uright) ? P.projXR[i] : 0.f;
                    for_window(F, Q, 0, Q.keys, nLeft, w, level - 1, level, lane, [&](const WinEntry &kp) {
                        if (!in_box(kp, x, y, rad, level - 1, level)) return;
                        const int idx = kp.idx;
                        const bool held = Q.holderObs[idx] > 0;
                        const bool locked = is_locked(C, idx, i, held);
                        if (locked && !cb.build) return;
                        if (kp.uright > 0) {  // (mono-stereo frames only: the records of other frames hold -1)
                            const float er = fabsf(__fsub_rn(pxr, kp.uright));
                            if (er > rad) return;
                        }
                        const int dist = hamming256(q, kp.d);
                        const unsigned long long key = make_key(dist, kp.cx, kp.cy, idx, kp.octave, held);
                        if (cb.build) cache_append(cb, key);
                        if (locked) return;
                        two_min_insert(k0, k1, key);
                    });
                }
                cache_end(cb, lane, false);
            }
            wave_two_min(k0, k1);
            if (k0 != KEY_NONE) {
                bd = key_dist(k0);
                bi = key_idx(k0);
                bl = key_octave(k0);
            }
            if (k1 != KEY_NONE) {
                bd2 = key_dist(k1);
                bl2 = key_octave(k1);
            }
            if (bd <= FT_TH_HIGH) {
                if (bl == bl2 && (float)bd > __fmul_rn(nnRatio, (float)bd2)) {
                    skipRight = true;  // the reference's `continue` also skips the right-camera block
                } else {
                    primL = bi;
                    if (F.Nleft != -1 && Q.l2r[bi] != -1) sideL = Q.l2r[bi] + F.Nleft;
                }
            }
        }
        if (twoCam && inViewRV && !skipRight) {
            const int level = levelRV;
            if (level != -1) {
                const int nRight = F.N - F.Nleft;
                unsigned long long k0 = KEY_NONE, k1 = KEY_NONE;
                // this point's own left-block side write precedes its right-block search
                auto lockedR = [&](int g, bool held) -> bool { return (g == sideL) ? (C.obs[i] > 0) : is_locked(C, g, i, held); };
                // (the right block is not reached in every pass - skipRight depends on the locks - so its candidates are filed by
                // the first pass that gets here)
                CacheBuild cb;
                cb.slot = slotR;
                cb.counter = ldsCounter;
                int nCached;
                bool anyBox;
                const int cs = slotR ? cache_state_of(metaR, nCached, anyBox) : 2;
                cb.build = cs == 0;
                if (cs == 1) {
                    for (int t = lane; t < nCached; t += 64) {
                        const unsigned long long key = t < 64 ? keyR0 : cb.slot[1 + t];
                        if (lockedR(key_idx(key) + F.Nleft, key_held(key))) continue;
                        two_min_insert(k0, k1, key);
                    }
                } else {
                    const float r = ((double)P.viewCosR[i] > 0.998) ? 2.5f : 4.0f;
                    const float rad = __fmul_rn(r, F.sf[level]);
                    const float x = P.projXR[i], y = P.projYR[i];
                    const Window w = cell_window(F, x, y, rad);
                    cache_begin(cb, lane);
                    if (!w.empty) {
                        for_window(F, Q, 1, Q.keysR, nRight, w, level - 1, level, lane, [&](const WinEntry &kp) {
                            if (!in_box(kp, x, y, rad, level - 1, level)) return;
                            const int idx = kp.idx, g = idx + F.Nleft;
                            const bool held = Q.holderObs[g] > 0;
                            const bool locked = lockedR(g, held);
                            if (locked && !cb.build) return;
                            const int dist = hamming256(q, kp.d);
                            const unsigned long long key = make_key(dist, kp.cx, kp.cy, idx, kp.octave, held);
                            if (cb.build) cache_append(cb, key);
                            if (locked) return;
                            two_min_insert(k0, k1, key);
                        });
                    }
                    cache_end(cb, lane, false);
                }
                wave_two_min(k0, k1);
                if (k0 != KEY_NONE) {
                    bdr = key_dist(k0);
                    bir = key_idx(k0);
                    blr = key_octave(k0);
                }
                if (k1 != KEY_NONE) {
                    bd2r = key_dist(k1);
                    bl2r = key_octave(k1);
                }
                if (bdr <= FT_TH_HIGH && !(blr == bl2r && (float)bdr > __fmul_rn(nnRatio, (float)bd2r))) {
                    if (Q.r2l[bir] != -1) sideR = Q.r2l[bir];
                    primR = bir + F.Nleft;
                }
            }
        }
    }
    r4[0] = primL; r4[1] = sideL; r4[2] = primR; r4[3] = sideR;
    if (lane == 0 && raw.bestDist) {  // the reference kernel's raw outputs are optional (the resident-frame path skips them)
        raw.bestDist[i] = bd; raw.bestDist2[i] = bd2; raw.bestLevel[i] = bl; raw.bestLevel2[i] = bl2; raw.bestIdx[i] = bi;
        raw.bestDistR[i] = bdr; raw.bestDist2R[i] = bd2r; raw.bestLevelR[i] = blr; raw.bestLevel2R[i] = bl2r; raw.bestIdxR[i] = bir;
    }
}

// waves (= points) per workgroup of the search kernels: a pass is short, and its fixed cost is the dispatch of its workgroups
#ifndef FT_SEARCH_WPB
#define FT_SEARCH_WPB 4
#endif
__global__ __launch_bounds__(64 * FT_SEARCH_WPB) void k_search_local(FtDevFrame F, FtDevLocalPoints P, FtClaims C, float th,
                                                      float nnRatio, int *res, FtLocalRaw raw) {
    if (!claims_begin_pass(C)) return;
    const int lane = threadIdx.x & 63, wave = wave_index();
    const int i = blockIdx.x * FT_SEARCH_WPB + wave;
    if (i >= P.M) return;
    __shared__ int cacheCounter[FT_SEARCH_WPB];
    int r4[4];
    local_point(F, frame_ptrs(F, FT_NO_REBASE), P, C, th, nnRatio, i, lane, r4, raw, &cacheCounter[wave]);
    claims_file(C, res, i, lane, r4);
}

// ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for last-frame point i by one wave (src/ORBmatcher.cc:
// 1775-1960): r = (left keypoint written, -1, right keypoint written, -1)
// pre (may be null): the projections of the points, computed once per point by k_last_project_batch - the pose transform and the
// camera model (two atan2f, a cosf and a sinf per camera for KannalaBrandt8) are the same number in all 64 lanes of a point's wave
template <bool PRE = false>
__device__ __forceinline__ void last_point(const FtDevFrame &F, const FramePtrs &Q, const FtDevLastPoints &Lp, const FtClaims &C, const FtPose &Tcw,
                                           float th, int bForward, int bBackward, int i, int lane, int r4[4], const FtLastRaw &raw,
                                           int *ldsCounter, const FtLastProj *pre = nullptr) {
    int primL = -1, primR = -1;
    int bd = 256, bi = -1, bdr = 256, bir = -1;
    // Later passes of the claim iteration on a point whose candidates are cached need neither the pose transform nor the camera
    // model (two atan2f, a cosf and a sinf for KannalaBrandt8 - evaluated by all 64 lanes, on the critical path of a pass that
    // is otherwise a handful of dependent loads): the cached keys already hold everything that depends on the projection.
    unsigned long long *slotL = C.cache ? C.cache + (size_t)i * FT_CACHE_WORDS : nullptr;
    unsigned long long *slotR = slotL ? slotL + (FT_CACHE_CAP + 1) : nullptr;
    // requested together, before the first use: validity, both meta words and (speculatively) the first 64 keys of either camera
    const bool twoCam = F.Nleft != -1;
    const uint8_t validV = Lp.valid[i];
    const unsigned long long metaL = slotL ? slotL[0] : KEY_NONE, metaR = (slotR && twoCam) ? slotR[0] : KEY_NONE;
    const unsigned long long keyL0 = slotL ? slotL[1 + lane] : KEY_NONE, keyR0 = (slotR && twoCam) ? slotR[1 + lane] : KEY_NONE;
    bool fromCache = false;
    int nCachedL = 0, nCachedR = 0;
    bool anyBoxL = false, anyBoxR = false;
    if (validV && slotL && cache_state_of(metaL, nCachedL, anyBoxL) == 1)
        fromCache = !twoCam || !anyBoxL || cache_state_of(metaR, nCachedR, anyBoxR) == 1;
    if (fromCache) {
        unsigned long long k0 = KEY_NONE;
        for (int t = lane; t < nCachedL; t += 64) {
            const unsigned long long key = t < 64 ? keyL0 : slotL[1 + t];
            if (is_locked(C, key_idx(key), i, key_held(key))) continue;
            k0 = key < k0 ? key : k0;
        }
        k0 = wave_min_u64(k0);
        if (anyBoxL) {
            if (k0 != KEY_NONE) {
                bd = key_dist(k0);
                bi = key_idx(k0);
            }
            if (bd <= FT_TH_HIGH) primL = bi;
            if (F.Nleft != -1) {
                unsigned long long kr = KEY_NONE;
                for (int t = lane; t < nCachedR; t += 64) {
                    const unsigned long long key = t < 64 ? keyR0 : slotR[1 + t];
                    if (is_locked(C, key_idx(key) + F.Nleft, i, key_held(key))) continue;
                    kr = key < kr ? key : kr;
                }
                kr = wave_min_u64(kr);
                if (kr != KEY_NONE) {
                    bdr = key_dist(kr);
                    bir = key_idx(kr);
                }
                if (bdr <= FT_TH_HIGH) primR = bir + F.Nleft;
            }
        }
    } else if (validV) {
        float xc[3] = {0.f, 0.f, 0.f}, uv[2] = {0.f, 0.f}, uvrPre[2] = {0.f, 0.f};
        float invzc;
        bool go;
        if constexpr (PRE) {
            const FtLastProj pj = pre[i];
            uv[0] = pj.u; uv[1] = pj.v; invzc = pj.invzc; uvrPre[0] = pj.ur; uvrPre[1] = pj.vr;
            go = pj.go != 0;
        } else {
            float xw[3] = {Lp.worldPos[3 * i], Lp.worldPos[3 * i + 1], Lp.worldPos[3 * i + 2]};
            transform_pose(Tcw.m, Tcw.q, Tcw.quat, xw, xc);
            invzc = (float)(1.0 / (double)xc[2]);
            go = !(invzc < 0);
            if (go) {
                project_cam(F, xc, uv);
                if (uv[0] < F.mnMinX || uv[0] > F.mnMaxX) go = false;
                if (uv[1] < F.mnMinY || uv[1] > F.mnMaxY) go = false;
            }
        }
        // a point that does not project into the image: an empty cache entry spares the later passes the projection
        if (!go && slotL && lane == 0 && metaL == KEY_NONE) slotL[0] = 0ull;
        if (go) {
            const int oct = Lp.octave[i];
            const float radius = __fmul_rn(th, F.sf[oct]);
            int minLevel, maxLevel;
            if (bForward) { minLevel = oct; maxLevel = -1; }
            else if (bBackward) { minLevel = 0; maxLevel = oct; }
            else { minLevel = oct - 1; maxLevel = oct + 1; }
            unsigned long long q[4];
            {
                const unsigned long long *p = (const unsigned long long *)(Lp.desc + (size_t)i * 32);
                q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = p[3];
            }
            const int nLeft = F.Nleft == -1 ? F.N : F.Nleft;
            const Window w = cell_window(F, uv[0], uv[1], radius);
            unsigned long long k0 = KEY_NONE;
            int anyCand = 0;
            CacheBuild cb;
            cb.slot = C.cache ? C.cache + (size_t)i * FT_CACHE_WORDS : nullptr;
            cb.counter = ldsCounter;
            int nCached;
            bool anyBox;
            const int cs = cache_state(cb.slot, nCached, anyBox);
            cb.build = cs == 0;
            if (cs == 1) {
                anyCand = anyBox ? 1 : 0;
                for (int t = lane; t < nCached; t += 64) {
                    const unsigned long long key = cb.slot[1 + t];
                    if (is_locked(C, key_idx(key), i, key_held(key))) continue;
                    k0 = key < k0 ? key : k0;
                }
            } else {
                cache_begin(cb, lane);
                if (!w.empty) {
                    for_window(F, Q, 0, Q.keys, nLeft, w, minLevel, maxLevel, lane, [&](const WinEntry &kp) {
                        if (!in_box(kp, uv[0], uv[1], radius, minLevel, maxLevel)) return;
                        anyCand = 1;
                        const int idx = kp.idx;
                        const bool held = Q.holderObs[idx] > 0;
                        const bool locked = is_locked(C, idx, i, held);
                        if (locked && !cb.build) return;
                        if (kp.uright > 0) {
                            const float ur = __fsub_rn(uv[0], __fmul_rn(F.mbf, invzc));
                            const float er = fabsf(__fsub_rn(ur, kp.uright));
                            if (er > radius) return;
                        }
                        const int dist = hamming256(q, kp.d);
                        const unsigned long long key = make_key(dist, kp.cx, kp.cy, idx, kp.octave, held);
                        if (cb.build) cache_append(cb, key);
                        if (locked) return;
                        k0 = key < k0 ? key : k0;
                    });
                }
                anyCand = __any(anyCand);
                cache_end(cb, lane, anyCand != 0);
            }
            k0 = wave_min_u64(k0);
            // `if(vIndices2.empty()) continue;` (ORBmatcher.cc:1836) also skips the right-camera block
            if (anyCand) {
                if (k0 != KEY_NONE) {
                    bd = key_dist(k0);
                    bi = key_idx(k0);
                }
                if (bd <= FT_TH_HIGH) primL = bi;
                if (F.Nleft != -1) {
                    float xr[3], uvr[2];
                    if constexpr (PRE) {
                        uvr[0] = uvrPre[0];
                        uvr[1] = uvrPre[1];
                    } else {
                        transform_pose(F.Trl, F.TrlQ, F.trlQuat, xc, xr);
                        project_cam(F, xr, uvr);
                    }
                    const Window wr = cell_window(F, uvr[0], uvr[1], radius);
                    const int nRight = F.N - F.Nleft;
                    unsigned long long kr = KEY_NONE;
                    CacheBuild cbr;
                    cbr.slot = C.cache ? C.cache + (size_t)i * FT_CACHE_WORDS + (FT_CACHE_CAP + 1) : nullptr;
                    cbr.counter = ldsCounter;
                    int nCachedR;
                    bool anyBoxR;
                    const int csr = cache_state(cbr.slot, nCachedR, anyBoxR);
                    cbr.build = csr == 0;
                    if (csr == 1) {
                        for (int t = lane; t < nCachedR; t += 64) {
                            const unsigned long long key = cbr.slot[1 + t];
                            if (is_locked(C, key_idx(key) + F.Nleft, i, key_held(key))) continue;
                            kr = key < kr ? key : kr;
                        }
                    } else {
                        cache_begin(cbr, lane);
                        if (!wr.empty) {
                            for_window(F, Q, 1, Q.keysR, nRight, wr, minLevel, maxLevel, lane, [&](const WinEntry &kp) {
                                if (!in_box(kp, uvr[0], uvr[1], radius, minLevel, maxLevel)) return;
                                const int idx = kp.idx;
                                const bool held = Q.holderObs[idx + F.Nleft] > 0;
                                const bool locked = is_locked(C, idx + F.Nleft, i, held);
                                if (locked && !cbr.build) return;
                                const int dist = hamming256(q, kp.d);
                                const unsigned long long key = make_key(dist, kp.cx, kp.cy, idx, kp.octave, held);
                                if (cbr.build) cache_append(cbr, key);
                                if (locked) return;
                                kr = key < kr ? key : kr;
                            });
                        }
                        cache_end(cbr, lane, false);
                    }
                    kr = wave_min_u64(kr);
                    if (kr != KEY_NONE) {
                        bdr = key_dist(kr);
                        bir = key_idx(kr);
                    }
                    if (bdr <= FT_TH_HIGH) primR = bir + F.Nleft;
                }
            }
        }
    }
    r4[0] = primL; r4[1] = -1; r4[2] = primR; r4[3] = -1;
    if (lane == 0 && raw.bestDist) {
        raw.bestDist[i] = bd; raw.bestIdx[i] = bi; raw.bestDistR[i] = bdr; raw.bestIdxR[i] = bir;
    }
}

__global__ __launch_bounds__(64 * FT_SEARCH_WPB) void k_search_last(FtDevFrame F, FtDevLastPoints Lp, FtClaims C, FtPose Tcw, float th,
                                                     int bForward, int bBackward, int *res, FtLastRaw raw) {
    if (!claims_begin_pass(C)) return;
    const int lane = threadIdx.x & 63, wave = wave_index();
    const int i = blockIdx.x * FT_SEARCH_WPB + wave;
    if (i >= Lp.N) return;
    __shared__ int cacheCounter[FT_SEARCH_WPB];
    int r4[4];
    last_point(F, frame_ptrs(F, FT_NO_REBASE), Lp, C, Tcw, th, bForward, bBackward, i, lane, r4, raw, &cacheCounter[wave]);
    claims_file(C, res, i, lane, r4);
}

// the projections of SearchByProjection(CurrentFrame, LastFrame) once per point (thread per point, blockIdx.y = frame): exactly the
// expressions of last_point - Tcw * x3Dw, 1 / z, mpCamera->project, the bounds test, and for two-camera frames Trl * x3Dc and
// mpCamera2->project (src/ORBmatcher.cc:1805-1822, 1900-1902)
__global__ __launch_bounds__(256) void k_last_project_batch(const FtBatchJob *__restrict__ jobs, Rebase rb) {
    const FtBatchJob &J = jobs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= J.L.N || J.nPoints <= 0) return;
    const FtDevFrame &F = J.F;
    FtLastProj pj;
    pj.u = pj.v = pj.invzc = pj.ur = pj.vr = 0.f;
    pj.go = 0;
    uint8_t *valid = const_cast<uint8_t *>(rb(J.L.valid));
    // a valid point's octave indexes the frame's scale factors in every kernel behind this one: a value outside the levels
    // (the host checks it when it copies the points; arrays read in place from pinned memory are checked here) drops the point
    // and marks the frame - the call's second half reports FT_ERR_INVALID
    if (valid[i] && ((unsigned)rb(J.L.octave)[i] >= (unsigned)F.nlevels)) {
        valid[i] = 0;
        int *err = rb(J.err);
        if (err) atomicOr(err, FT_JOB_ERR_OCTAVE);
    }
    if (valid[i]) {
        const float *wp = rb(J.L.worldPos);
        const float xw[3] = {wp[3 * i], wp[3 * i + 1], wp[3 * i + 2]};
        float xc[3], uv[2] = {0.f, 0.f};
        transform_pose(J.Tcw.m, J.Tcw.q, J.Tcw.quat, xw, xc);
        const float invzc = (float)(1.0 / (double)xc[2]);
        bool go = !(invzc < 0);
        if (go) {
            project_cam(F, xc, uv);
            if (uv[0] < F.mnMinX || uv[0] > F.mnMaxX) go = false;
            if (uv[1] < F.mnMinY || uv[1] > F.mnMaxY) go = false;
        }
        pj.u = uv[0]; pj.v = uv[1]; pj.invzc = invzc;
        pj.go = go ? 1 : 0;
        if (go && F.Nleft != -1) {
            float xr[3], uvr[2];
            transform_pose(F.Trl, F.TrlQ, F.trlQuat, xc, xr);
            project_cam(F, xr, uvr);
            pj.ur = uvr[0]; pj.vr = uvr[1];
        }
    }
    rb(J.proj)[i] = pj;
}

// ---- B frames per launch (ft_tracked_batch): blockIdx.y = frame, the pass's buffers from the frame's job (job_claims, search_dev.h) ----
// slowList != 0: a later pass - the points the lean kernel (k_search_*_lean, kernels_search_rows.hip) could not serve from the
// candidate cache, by a grid-stride loop over the frame's slow list of this pass's parity; the pass's clears were done by the lean kernel
#ifndef FT_BATCH_WAVES
#define FT_BATCH_WAVES 6  // waves per SIMD the first-pass kernels are compiled for (80 registers, 12 - 32 bytes of scratch: 0.60 -> 0.545 ms; 8: spills, 0.82 ms)
#endif
template <bool slowList>
__global__ __launch_bounds__(64 * FT_SEARCH_WPB) __attribute__((amdgpu_waves_per_eu(FT_BATCH_WAVES, 8))) void k_search_last_batch(const FtBatchJob *__restrict__ jobs, Rebase rb, int pass, int fCur,
                                                                          int fPrev, int fReset, float th) {
    const FtBatchJob &J = jobs[blockIdx.y];
    if (J.nPoints <= 0) return;
    int *res;
    const FtClaims C = job_claims(J, rb, pass, fCur, fPrev, fReset, res);
    const int lane = threadIdx.x & 63, wave = wave_index();
    __shared__ int cacheCounter[FT_SEARCH_WPB];
    const FtLastRaw raw = {nullptr, nullptr, nullptr, nullptr};
    FtDevLastPoints L = J.L;
    L.valid = rb(L.valid); L.worldPos = rb(L.worldPos); L.desc = rb(L.desc); L.octave = rb(L.octave);
    const FramePtrs Q = frame_ptrs(J.F, rb);
    if constexpr (!slowList) {
        if (!claims_begin_pass(C)) return;
        const int i = blockIdx.x * FT_SEARCH_WPB + wave;
        if (i >= J.L.N) return;
        int r4[4];
        last_point<true>(J.F, Q, L, C, J.Tcw, th, J.forward, J.backward, i, lane, r4, raw, &cacheCounter[wave], rb(J.proj));
        claims_file(C, res, i, lane, r4);
        return;
    } else {
    if (C.flagPrev && shared_load(C.flagPrev) == -1) return;
    const int *slow = rb(J.slow);
    const int count = slow[pass & 1];
    for (int k = blockIdx.x * FT_SEARCH_WPB + wave; k < count; k += gridDim.x * FT_SEARCH_WPB) {
        const int i = slow[16 + (size_t)(pass & 1) * J.nPoints + k];
        int r4[4];
        last_point<true>(J.F, Q, L, C, J.Tcw, th, J.forward, J.backward, i, lane, r4, raw, &cacheCounter[wave], rb(J.proj));
        claims_file(C, res, i, lane, r4);
    }
    }
}

template <bool slowList>
__global__ __launch_bounds__(64 * FT_SEARCH_WPB) __attribute__((amdgpu_waves_per_eu(FT_BATCH_WAVES, 8))) void k_search_local_batch(const FtBatchJob *__restrict__ jobs, Rebase rb, int pass, int fCur,
                                                                           int fPrev, int fReset, float th, float nnRatio) {
    const FtBatchJob &J = jobs[blockIdx.y];
    if (J.nPoints <= 0) return;
    int *res;
    const FtClaims C = job_claims(J, rb, pass, fCur, fPrev, fReset, res);
    const int lane = threadIdx.x & 63, wave = wave_index();
    __shared__ int cacheCounter[FT_SEARCH_WPB];
    FtLocalRaw raw;
    raw.bestDist = nullptr;
    FtDevLocalPoints P = J.P;
    P.skip = rb(P.skip); P.inView = rb(P.inView); P.inViewR = rb(P.inViewR);
    P.level = rb(P.level); P.levelR = rb(P.levelR);
    P.viewCos = rb(P.viewCos); P.viewCosR = rb(P.viewCosR);
    P.projX = rb(P.projX); P.projY = rb(P.projY); P.projXR = rb(P.projXR); P.projYR = rb(P.projYR);
    P.desc = rb(P.desc);
    const FramePtrs Q = frame_ptrs(J.F, rb);
    if constexpr (!slowList) {
        if (!claims_begin_pass(C)) return;
        const int i = blockIdx.x * FT_SEARCH_WPB + wave;
        if (i >= J.P.M) return;
        int r4[4];
        local_point(J.F, Q, P, C, th, nnRatio, i, lane, r4, raw, &cacheCounter[wave]);
        claims_file(C, res, i, lane, r4);
        return;
    } else {
    if (C.flagPrev && shared_load(C.flagPrev) == -1) return;
    const int *slow = rb(J.slow);
    const int count = slow[pass & 1];
    for (int k = blockIdx.x * FT_SEARCH_WPB + wave; k < count; k += gridDim.x * FT_SEARCH_WPB) {
        const int i = slow[16 + (size_t)(pass & 1) * J.nPoints + k];
        int r4[4];
        local_point(J.F, Q, P, C, th, nnRatio, i, lane, r4, raw, &cacheCounter[wave]);
        claims_file(C, res, i, lane, r4);
    }
    }
}

}  // namespace

int ft_launch_features_in_area(hipStream_t st, const FtDevFrame &F, int nq, const float *qx, const float *qy, const float *qr,
                               const int *qmin, const int *qmax, const uint8_t *qright, const int *offsets,
                               unsigned *outKeys, int *outCount) {
    if (nq <= 0) return FT_OK;
    hipLaunchKernelGGL(k_features_in_area, dim3((nq + 3) / 4), dim3(256), 0, st, F, nq, qx, qy, qr, qmin, qmax, qright, offsets,
                       outKeys, outCount);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_search_local(hipStream_t st, const FtDevFrame &F, const FtDevLocalPoints &P, const FtClaims &C, float th,
                           float nnRatio, int *res, const FtLocalRaw &raw) {
    if (P.M <= 0) return FT_OK;
    hipLaunchKernelGGL(k_search_local, dim3((P.M + FT_SEARCH_WPB - 1) / FT_SEARCH_WPB), dim3(64 * FT_SEARCH_WPB), 0, st, F, P, C, th, nnRatio, res, raw);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_search_last(hipStream_t st, const FtDevFrame &F, const FtDevLastPoints &L, const FtClaims &C,
                          const FtPose &Tcw, float th, int forward, int backward, int *res, const FtLastRaw &raw) {
    if (L.N <= 0) return FT_OK;
    hipLaunchKernelGGL(k_search_last, dim3((L.N + FT_SEARCH_WPB - 1) / FT_SEARCH_WPB), dim3(64 * FT_SEARCH_WPB), 0, st, F, L, C, Tcw, th, forward, backward, res, raw);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

// ---- launches of a batch of frames (ft_tracked_batch, tracked_batch.cpp) ----
#define FT_SLOW_BLOCKS 16  // workgroups per frame of a slow-list launch (a grid-stride loop serves longer lists)

// the points' projections, once per search (J.proj; every pass and the slow lists read them): on its own for the first pass
// with four points per wave (ft_launch_search_last_first, kernels_search_rows.hip)
int ft_launch_last_project_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints) {
    if (nFrames <= 0 || maxPoints <= 0) return FT_OK;
    hipLaunchKernelGGL(k_last_project_batch, dim3((maxPoints + 255) / 256, nFrames), dim3(256), 0, st, jobs, rebase_of(arena));
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_search_last_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints, int pass, int fCur, int fPrev,
                                int fReset, float th) {
    if (nFrames <= 0 || maxPoints <= 0) return FT_OK;
    if (pass == 0)  // the points' projections, once (J.proj; the later passes and the slow lists read them too)
        hipLaunchKernelGGL(k_last_project_batch, dim3((maxPoints + 255) / 256, nFrames), dim3(256), 0, st, jobs, rebase_of(arena));
    hipLaunchKernelGGL(k_search_last_batch<false>, dim3((maxPoints + FT_SEARCH_WPB - 1) / FT_SEARCH_WPB, nFrames), dim3(64 * FT_SEARCH_WPB), 0, st,
                       jobs, rebase_of(arena), pass, fCur, fPrev, fReset, th);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_search_local_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints, int pass, int fCur, int fPrev,
                                 int fReset, float th, float nnRatio) {
    if (nFrames <= 0 || maxPoints <= 0) return FT_OK;
    hipLaunchKernelGGL(k_search_local_batch<false>, dim3((maxPoints + FT_SEARCH_WPB - 1) / FT_SEARCH_WPB, nFrames), dim3(64 * FT_SEARCH_WPB), 0,
                       st, jobs, rebase_of(arena), pass, fCur, fPrev, fReset, th, nnRatio);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

// the general kernel on the slow lists of a later pass, behind the lean kernel (ft_launch_search_*_batch_lean, kernels_search_rows.hip)
int ft_launch_search_last_batch_slow(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int pass, int fCur, int fPrev, int fReset,
                                     float th) {
    hipLaunchKernelGGL(k_search_last_batch<true>, dim3(FT_SLOW_BLOCKS, nFrames), dim3(64 * FT_SEARCH_WPB), 0, st, jobs, rebase_of(arena), pass,
                       fCur, fPrev, fReset, th);
    FT_HIP(hipGetLastError());
    return FT_OK;
}
int ft_launch_search_local_batch_slow(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int pass, int fCur, int fPrev, int fReset,
                                      float th, float nnRatio) {
    hipLaunchKernelGGL(k_search_local_batch<true>, dim3(FT_SLOW_BLOCKS, nFrames), dim3(64 * FT_SEARCH_WPB), 0, st, jobs, rebase_of(arena), pass,
                       fCur, fPrev, fReset, th, nnRatio);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

// Device-side views used by the projection-search kernels (kernels_search.hip, kernels_search_rows.hip, kernels_resolve.hip,
// kernels_frame.hip) and their host side (search_host.h), and the launches of those kernels.
#pragma once

#include "ft_internal.h"
#include "fv_host.h"

struct FtDevFrame {
    int N, Nleft;
    float mnMinX, mnMinY, mnMaxX, mnMaxY, invW, invH, mbf, mb;
    const ft_keypoint *keys, *keysR;  // device
    const uint8_t *desc;              // device N x 32
    const float *uright;              // device or null
    const int *holderObs;             // device [N] pre-call Observations() of mvpMapPoints[i] (-1 = none)
    const int *l2r, *r2l;             // device or null
    int camModel;
    float cam[8];
    float Trl[12];
    float TrlQ[4];  // trlQuat != 0: GetRelativePoseTrl() in the Sophus form (translation in Trl[3], [7], [11])
    int trlQuat;
    float sf[FT_MAX_LEVELS];
    int nlevels;
    // Frame::mGrid as one CSR per octave (k_build_grid; AssignFeaturesToGrid src/Frame.cc:409-440): the keypoints of octave o
    // in cell (cx, cy) are the entries gridStart[o * (FT_GRID_CELLS + 1) + cx * 48 + cy] .. [... + 1), so the part of a
    // window's column cx that lies in the search's level band is ONE contiguous range per octave; [0] left camera (or the
    // only one), [1] right camera.  Null = no grid: the searches then scan every keypoint.
    const int *gridStart[2];
    // the entries as search records {x, y, uright (or -1), index | octave << 24} and 32-byte descriptors - what a window
    // scan needs of a keypoint, as two contiguous reads per run of entries instead of the chain grid entry -> keypoint ->
    // descriptor / uright
    const float4 *gridRec[2];
    const uint8_t *gridDesc[2];
};
#define FT_GRID_CELLS (FT_GRID_COLS * FT_GRID_ROWS)

struct FtDevLocalPoints {
    int M;
    const uint8_t *skip, *inView, *inViewR;
    const int *level, *levelR;
    const float *viewCos, *viewCosR, *projX, *projY, *projXR, *projYR;
    const uint8_t *desc;
};

struct FtDevLastPoints {
    int N;
    const uint8_t *valid;
    const float *worldPos;
    const uint8_t *desc;
    const int *octave;
    const float *angle;  // batch form only: the last-frame keypoints' angles (rotation histogram of k_replay_batch), may be null
};

// The claim iteration (Jacobi passes over the sequential claiming of SearchByProjection): a pass reads the writer lists
// the previous pass built - head[kp] -> slot s (= 4 * point + write kind), next[s] - and builds the lists of the next
// pass while it runs, so a pass is ONE launch.  The list heads rotate through three arrays (read / write / clear), next
// and the results through two.  Flags: -1 = "this pass changed nothing", 0 = "changed" (one memset with 0xff prepares
// heads and flags of a call); a pass returns at once when the previous pass's flag says the fixed point was reached.
struct FtClaims {
    const int *head, *next;  // writer lists of the previous pass
    const int *obs;          // Observations() per map point
    int firstPass;           // no lists yet: the pre-call holders decide, and every result counts as changed
    int *headWrite, *nextWrite;  // lists this pass builds for the next one
    int *headClear;          // the heads the next pass will write: reset to -1 here
    // the writer table (search_dev.h, FT_TAB_ENTRIES): 8 ints per keypoint, rotating like the heads; head / next
    // only take the writers a record has no room for
    const int *tab;
    int *tabWrite, *tabClear;
    int nKp;
    const int *resPrev;      // results of the previous pass
    int *flagCur;            // this pass's flag (atomicAnd 0 on a change)
    const int *flagPrev;     // the previous pass's flag (null for the first pass of a burst)
    int *flagReset;          // the flag of the same position in the other burst parity: reset to -1 here
    int *flagStick = nullptr;  // batch form only: the 16 flag words of this burst (claims_begin_pass, search_dev.h)
    // Candidate cache (may be null).  What does NOT change from pass to pass - which keypoints of a point's window pass the
    // level band, the box and the uright test, and their Hamming distances - is computed once: the first pass that reaches a
    // (point, camera) window files the (distance, cell x, cell y, index) keys of all its candidates here, and every later
    // pass only walks those keys against the new lock state (a round of 64 keys = one coalesced load + the lock look-ups)
    // instead of walking the grid, the keypoints and the descriptors again.  A pass of the iteration is as long as its
    // slowest wave, and a window scan is a chain of ~5 dependent loads per 64 entries: 85 us per pass at th 15, whatever
    // the number of points.  Per (point, camera) FT_CACHE_CAP + 1 64-bit words: [0] = ~0 "not built" | number of
    // candidates (more than FT_CACHE_CAP: not cached, scan again) | any keypoint in the box << 32, then the keys, unordered.
    unsigned long long *cache;
};
#ifndef FT_CACHE_CAP
#define FT_CACHE_CAP 511
#endif
#define FT_CACHE_WORDS (2 * (FT_CACHE_CAP + 1))  // per point: left and right camera

// a rigid transform: row-major 3x4 (y = R x + t), or - quat != 0 - as Sophus::SE3f holds and applies it: unit quaternion
// q = (x, y, z, w), translation in m[3], m[7], m[11] (transform_pose, search_dev.h)
struct FtPose {
    float m[12];
    float q[4];
    int quat;
};

struct FtLocalRaw {
    int *bestDist, *bestDist2, *bestLevel, *bestLevel2, *bestIdx;
    int *bestDistR, *bestDist2R, *bestLevelR, *bestLevel2R, *bestIdxR;
};
struct FtLastRaw {
    int *bestDist, *bestIdx, *bestDistR, *bestIdxR;
};

// Frame::isInFrustum inputs / outputs (kernels_frame.hip k_frustum)
struct FtDevMapPoints {
    int M;
    const uint8_t *skip;  // may be null
    const float *worldPos, *normal, *maxDist, *minDist;
};
struct FtFrustumPose {
    float R[2][9], t[2][3], twc[2][3];  // [0] left camera (mRcw, mtcw, mOw), [1] right camera (Frame.cc:1314-1320)
};
struct FtFrustumOut {
    uint8_t *inView, *inViewR;
    int *level, *levelR;
    float *viewCos, *viewCosR, *projX, *projY, *projXR, *projYR, *depth, *depthR;
    uint8_t *searchSkip;  // may be null: the `continue` conditions of ORBmatcher.cc:66-74 for the search that follows
    int *count;           // nToMatch (atomic; zeroed by the launcher)
};

// One frame of a batch of searches (ft_tracked_batch, tracked_batch.cpp): what the batch kernels read of frame blockIdx.y, resident
// in HBM.  Every pointer of a job points into the device arena of its batch (`arena` of the launchers below: the kernels
// re-derive the pointers from it, see FramePtrs in search_dev.h).  The rotating buffers of the claim iteration are addressed by pass number (job_claims, search_dev.h):
// res 2 x 4 nPoints | head 3 x K | next 2 x 4 nPoints | tab 3 x 8 K (K = keypoints rounded up to 8) | flags FT_BATCH_FLAGS.
// projection of a last-frame point into the current frame's camera(s) (k_last_project_batch, kernels_search.hip)
struct FtLastProj {
    float u, v, invzc, ur, vr;
    int go;  // projects into the image (src/ORBmatcher.cc:1807-1822)
};
#define FT_BATCH_FLAGS 64  // flag words per frame of a batch: two burst parities x 32 positions (a power of two)
struct FtBatchJob {
    FtDevFrame F;
    int *res, *head, *next, *tab, *flags;
    int *slow;                  // [0], [1]: lengths of the slow lists of even / odd passes, then 2 x nPoints entries from word 16
    const int *obs;             // Observations() per point of the running search
    unsigned long long *cache;  // FT_CACHE_WORDS per point, or null
    int K, nKp, nPoints;
    // SearchByProjection(CurrentFrame, LastFrame)
    FtDevLastPoints L;
    FtPose Tcw;
    int forward, backward;
    FtLastProj *proj;  // [L.N], written by the first pass's projection launch
    // isInFrustum + SearchByProjection(Frame, local map points)
    FtDevMapPoints MP;
    FtFrustumPose T;
    FtFrustumOut O;
    FtDevLocalPoints P;
    // what the search leaves behind (k_replay_batch): assignOut [F.N] and nmOut [1] are PINNED HOST memory the kernel writes
    // directly (not in the arena: never rebased), replayed [1] (arena) is the frame's "done" marker: -1 until the frame's writes
    // have been replayed, then its match count
    int *assignOut, *nmOut, *replayed;
    int *err;  // [1] (arena), zeroed with the claim buffers: an input error a kernel found (FT_JOB_ERR_*), reported by the call's second half
};
#define FT_JOB_ERR_OCTAVE 1  // a valid last-frame point whose octave lies outside the frame's levels (the point is dropped)

// a block of bytes of PINNED HOST memory (the caller's arrays, read in place) gathered into the batch's arena by k_gather_batch
struct FtGatherRec {
    void *dst;        // device (arena)
    const void *src;  // pinned host
    unsigned bytes;
};
int ft_launch_gather_batch(hipStream_t st, const FtGatherRec *recs, int nRecs);
// a block of dwords delivered into pinned host memory by k_deliver_batch; src[parity of the last pass]
struct FtDeliverRec {
    void *dst;
    const void *src[2];
    int words;
};
// what two extractors left in HBM (slot slot0L + f / slot0R + f = left / right image of frame f of the batch), the lapping areas, and the
// per-frame (monoLeft, monoRight) counts the gather leaves for the matching
struct FtBindArgs {
    const ft_keypoint *keysL, *keysR;
    const uint8_t *descL, *descR;
    int strideL, strideR;  // keypoints per slot
    int slot0L, slot0R;  // first slot of the left / right extractor (one extractor may serve both cameras: disjoint slot ranges)
    int lapL0, lapL1, lapR0, lapR1;
    int *mono;  // [nFrames][2], device
    // the triangulation filter of Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1256-1271): 0 = the matching alone
    int triangulate;
    FtFisheyeRig rig;
    int *nMatches;      // [nFrames], device (zeroed by the gather)
    float *const *depth, *const *p3d;  // device tables of per-frame device arrays (mvDepth [Nleft], mvStereo3Dpoints [3 Nleft]), or null
};
// keypoints / descriptors of every frame into the reference's order, then the 2-NN + ratio matching of the lapping subsets
int ft_launch_bind_fisheye_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxKp, const FtBindArgs &A);
// KannalaBrandt8::TriangulateMatches for every ratio-test survivor of every frame (kernels_fisheye.hip): keeps mvLeftToRightMatch
// where the depth is > 0.0001, fills mvRightToLeftMatch, mvDepth, mvStereo3Dpoints and the frame's match count
int ft_launch_fisheye_triangulate_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxKp, const FtBindArgs &A);
int ft_launch_fill_claims_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxWords);
// behind the first pass of a batch: every candidate list with its best candidates at the front (cache_partition, kernels_search_rows.hip)
int ft_launch_cache_partition_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints);
int ft_launch_deliver_batch(hipStream_t st, const FtDeliverRec *recs, int nRecs, int maxWords, int parity);
int ft_launch_build_grid_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxLevels, bool twoCam);
int ft_launch_frustum_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxM, float viewingCosLimit, float logScaleFactor,
                            int farPoints, float thFar);
// one pass of the claim iteration of every frame; fCur / fPrev / fReset: positions in each frame's flag words (fPrev < 0: none)
int ft_launch_search_last_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints, int pass, int fCur, int fPrev,
                                int fReset, float th);
int ft_launch_search_local_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints, int pass, int fCur, int fPrev,
                                 int fReset, float th, float nnRatio);
// Parts of the launches below whose kernels live in kernels_search.hip (the launches themselves: kernels_search_rows.hip): the
// projections of the last-frame points in front of ft_launch_search_last_first, and the general kernel on the slow lists behind the
// lean kernel of ft_launch_search_*_batch_lean
int ft_launch_last_project_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints);
int ft_launch_search_last_batch_slow(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int pass, int fCur, int fPrev, int fReset,
                                     float th);
int ft_launch_search_local_batch_slow(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int pass, int fCur, int fPrev, int fReset,
                                      float th, float nnRatio);
// the first pass with four points per wave (a point = a row of 16 lanes): every frame needs its grid and the candidate cache;
// fills the lists, results and writer table exactly as pass 0 of ft_launch_search_*_batch does
int ft_launch_search_last_first(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints, float th);
int ft_launch_search_local_first(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints, float th, float nnRatio);
// everything behind that first pass in one launch: a workgroup per frame walks the frame's points in index order (k_resolve_batch);
// a frame it resolves has all its flag words at -1 and its results in both result buffers, a frame it gives up on is untouched
// sharedInts = ints of LDS for the frame's last-writer table (>= the largest F.N; <= 12288), 0 = frames beyond that: the table lives in HBM
int ft_launch_resolve_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int local, float nnRatio, int sharedInts);
// The writes of a converged search replayed on the device, a workgroup per frame (k_replay_batch): assign[keypoint] = the last
// point that wrote it, holder_obs updated in place in HBM, the match count; last frame: with the rotation histogram and
// ComputeThreeMaxima when checkOrientation.  Only frames that have not been replayed yet and - flagPos >= 0 - whose flag word at that
// position says "converged" (a launch enqueued before the host has looked: behind k_resolve_batch position 0, behind a burst of
// claim passes its last position; -1: every frame); parity = result buffer of the last pass (a converged frame holds its results in both).  sharedInts = ints of LDS per workgroup
// for the last-writer table (>= the largest F.N), 0 = frames too large for the LDS: the table lives in the frame's writer table
int ft_launch_replay_batch(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int local, int parity, int checkOrientation,
                           int sharedInts, int flagPos);
// a pass behind the first one: lean kernel (four points per wave from the candidate cache) + the general kernel on its slow list
int ft_launch_search_last_batch_lean(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints, int pass, int fCur,
                                     int fPrev, int fReset, float th);
int ft_launch_search_local_batch_lean(hipStream_t st, void *arena, const FtBatchJob *jobs, int nFrames, int maxPoints, int pass, int fCur,
                                      int fPrev, int fReset, float th, float nnRatio);
int ft_launch_fill_i32(hipStream_t st, int *p, int n, int v);
// p[0 .. n) = -1 and meta[i * strideWords] = ~0 for i < nMeta (meta may be null): the start of a claim iteration, one launch
int ft_launch_fill_claims(hipStream_t st, int *p, int n, unsigned long long *meta, int nMeta, int strideWords);
// p[i * strideWords] = v for i < n (64-bit words): the meta words of the candidate cache
int ft_launch_fill_stride_u64(hipStream_t st, unsigned long long *p, int n, int strideWords, unsigned long long v);
// one kernel copies up to three device blocks (sizes rounded up to dwords) into pinned host memory
int ft_launch_deliver_blocks(hipStream_t st, void *d0, const void *s0, size_t bytes0, void *d1, const void *s1, size_t bytes1,
                             void *d2, const void *s2, size_t bytes2);
int ft_launch_features_in_area(hipStream_t st, const FtDevFrame &F, int nq, const float *qx, const float *qy, const float *qr,
                               const int *qmin, const int *qmax, const uint8_t *qright, const int *offsets,
                               unsigned *outKeys, int *outCount);
int ft_launch_frustum(hipStream_t st, const FtDevFrame &F, const FtFrustumPose &T, const FtDevMapPoints &P,
                      float viewingCosLimit, float logScaleFactor, int farPoints, float thFar, const FtFrustumOut &O);
int ft_launch_search_local(hipStream_t st, const FtDevFrame &F, const FtDevLocalPoints &P, const FtClaims &C, float th,
                           float nnRatio, int *res, const FtLocalRaw &raw);
int ft_launch_search_last(hipStream_t st, const FtDevFrame &F, const FtDevLastPoints &L, const FtClaims &C,
                          const FtPose &Tcw, float th, int forward, int backward, int *res, const FtLastRaw &raw);
int ft_launch_build_grid(hipStream_t st, const FtDevFrame &F, int *gridStartL, int *gridStartR, float4 *recL, uint8_t *descL,
                         float4 *recR, uint8_t *descR);

// ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:747-862; kernels_init.hip).  A ROW is a level-0 keypoint of F1, in index
// order; an ORD is the rank of a level-0 keypoint of F2's grid in the order (cell column, cell row, index) - the order
// Frame::GetFeaturesInArea returns the keypoints of ANY window in, so "the first of equal distances" is "the smallest ord".
// A candidate is one word: distance << FT_INIT_ORD_BITS | ord.  cap1 / cap2 bound rows / ords (the host's counts of the
// level-0 keypoints): every table below has that many entries and no kernel writes beyond them.
#define FT_INIT_ORD_BITS 22
#define FT_INIT_NONE 0xffffffffu
#define FT_INIT_TOP 4  // candidates of a row the resolution looks at before it reads the row's segment
struct FtInitSearch {
    FtDevFrame F2;  // the current frame with its grid
    const ft_keypoint *keys1;
    const uint8_t *desc1;
    int N1;
    const float *prev;  // [N1][2] vbPrevMatched on entry
    float window, nnRatio;
    int checkOrientation;
    int cap1, cap2;
    int *counts;        // [0] rows, [1] ords (both clamped to the caps), [2] != 0: the device counted more than the caps admit
    int *rows;          // [cap1] keypoint of F1 of a row
    int *ordOfPos;      // [cap2] ord of the entry at position p of octave 0 of F2's grid
    int *idxOfOrd;      // [cap2] keypoint of F2 of an ord
    unsigned *seg;      // [cap1][cap2] the candidates of a row, unordered
    int *segCount;      // [cap1]
    unsigned *top;      // [cap1][FT_INIT_TOP] the smallest candidates of a row, ascending (FT_INIT_NONE = none)
    int *matches12;     // [N1]
    float *prevOut;     // [N1][2]
    int *matchedDist;   // [F2.N] vMatchedDistance (INT_MAX = unmatched)
    int *nMatches;      // [1]
};
// the three launches of a call, in this order; ldsBytes = 4 * (cap1 + cap2)
int ft_launch_init_prepare(hipStream_t st, const FtInitSearch &S);
int ft_launch_init_candidates(hipStream_t st, const FtInitSearch &S);
int ft_launch_init_resolve(hipStream_t st, const FtInitSearch &S);
#define FT_INIT_MAX_LDS (150 * 1024)

// ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:2087-2208;
// kernels_reloc.hip), the matcher of Tracking::Relocalization.  A POINT is an entry of pKF->GetMapPointMatches(), in index order.
// A candidate is a key (distance, cell x, cell y, index) as make_key (search_dev.h) builds it: ascending keys = ascending
// distance, then the order of Frame::GetFeaturesInArea.  Per point the FT_RELOC_TOP smallest keys (ascending) and a segment of
// FT_RELOC_SEG keys with all of them, unordered; a point with more candidates than the segment holds raises status[0] and the
// resolution writes nothing (FT_ERR_CAPACITY).
#define FT_RELOC_TOP 4
#define FT_RELOC_SEG 256
struct FtRelocProj {
    float u, v;
    int level;  // PredictScale
    int go;     // the point is searched (valid, projects into the image bounds, inside its distance range)
};
struct FtRelocSearch {
    FtDevFrame F;  // the current frame with its grid
    int N;         // points
    const uint8_t *valid;
    const float *worldPos, *maxDist, *minDist;
    const uint8_t *desc;
    const int *obs;
    const float *angle;  // may be null unless checkOrientation
    FtPose Tcw;          // Sophus form (quat != 0)
    float logScaleFactor, th;
    int orbDist, checkOrientation;
    FtRelocProj *proj;         // [N]
    unsigned long long *top;   // [N][FT_RELOC_TOP]
    unsigned long long *seg;   // [N][FT_RELOC_SEG]
    int *segCount;             // [N] candidates of a point (clamped to FT_RELOC_SEG)
    int *status;               // [0] != 0: a point has more candidates than its segment holds
    int *holder;               // [F.N] holder_obs of the frame, in / out (held on entry <=> != -1)
    int *assign;               // [F.N]
    int *bestDist, *bestIdx;   // [N]
    int *nMatches;             // [1]
};
// the three launches of a call, in this order
int ft_launch_reloc_project(hipStream_t st, const FtRelocSearch &S);
int ft_launch_reloc_candidates(hipStream_t st, const FtRelocSearch &S);
int ft_launch_reloc_resolve(hipStream_t st, const FtRelocSearch &S);
// dynamic LDS of the resolution: a taken bit per left keypoint and the keypoint a point took (<= FT_INIT_MAX_LDS)
inline size_t ft_reloc_lds_bytes(int nLeftKeys, int nPoints) { return 4 * (((size_t)nLeftKeys + 31) / 32 + (size_t)nPoints); }

// ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (src/ORBmatcher.cc:1006-1245;
// kernels_triang.hip) for keyframe 1 against every neighbour of a call.  Everything lives in ONE arena (what the host stages and
// copies up in one piece, then the outputs); a record holds byte offsets into it, so a kernel forms its addresses from the
// arena pointer it got as an argument.
#define FT_TRIANG_NONE 0xffffffffu  // FtTriangSide::uright: the keyframe has no mvuRight (all -1)
struct FtTriangSide {
    FtFv fv;                        // features and the FeatureVector in CSR form (fv_host.h)
    int nLeft;                      // KeyFrame::NLeft
    unsigned keys, desc;            // ft_keypoint[n], n x 32
    unsigned hasPoint, uright;      // uint8[n], float[n] (or FT_TRIANG_NONE)
    unsigned sf, sigma2;            // mvScaleFactors, mvLevelSigma2
    float cam[2][8];                // mpCamera, mpCamera2
};
struct FtTriangJob {  // one neighbour
    FtTriangSide K2;
    float ep[2], F12[9], R12[4][9], t12[4][3], precision;  // ft_triang_pair
    unsigned matches, bestDist;                            // int[K1.n] each
};
struct FtTriangCall {
    uint8_t *arena;
    FtTriangSide K1;
    unsigned k1;        // K1 once more, in the arena: what a lane selects by its own feature (the camera) is read from memory
    unsigned nodeOf;    // int[K1.n]: the FeatureVector entry that lists feature i, -1 = none (a stopped word)
    unsigned jobs;      // FtTriangJob[nNeighbours]
    unsigned nMatches;  // int[nNeighbours]
    int nNeighbours, camModel, twoCameras, onlyStereo, coarse, checkOrientation;
};
// the two launches of a call, in this order
int ft_launch_triang_match(hipStream_t st, const FtTriangCall &T);
int ft_launch_triang_finish(hipStream_t st, const FtTriangCall &T);

// The per-match text of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:483-692; kernels_newpoints.hip) on the match rows of
// the call above, in the same arena: what ft_newpoint_geometry adds to a keyframe, per neighbour the rows it writes.
struct FtNewPointSide {
    float Tcw[2][12], Ow[2][3];  // GetPose() / GetRightPose() as matrix3x4() row-major, GetCameraCenter() / GetRightCameraCenter()
    float Rwc[9], twc[3];        // mRwc, mTwc.translation() (KeyFrame::UnprojectStereo)
    float fx, fy, cx, cy, invfx, invfy, mb, mbf, precision;
    unsigned depth, keysRaw;     // float[n] mvDepth, ft_keypoint[n] mvKeys; FT_TRIANG_NONE: no stereo keypoint / the keys of the side
};
struct FtNewPointJob {  // one neighbour
    FtNewPointSide G2;
    unsigned status, x3d;  // int[K1.n], float[3 * K1.n]
};
struct FtNewPointCall {
    unsigned g1;              // FtNewPointSide of keyframe 1
    unsigned jobs;            // FtNewPointJob[nNeighbours]
    unsigned nPoints;         // int[nNeighbours], staged as 0: the workgroups of a neighbour add to it
    unsigned firstNeighbour;  // unsigned[K1.n], staged as 0xffffffff (-1): atomic minimum over the accepting neighbours
    int inertial, farPoints;
    float thFar, ratioFactor;
};
// one launch, behind ft_launch_triang_finish or on staged match rows: reads FtTriangJob::matches, FtTriangSide keys / uright / sf / sigma2 / cam
int ft_launch_triang_points(hipStream_t st, const FtTriangCall &T, const FtNewPointCall &P);

// One side of the batched SearchByBoW calls below in the arena of its call (stageBowSide, bow.cpp): records hold byte offsets into it.
// A side without a second camera - the frame of the candidate call among them - has nLeft = -1, nUn = n.
struct FtBowArenaSide {
    FtFv fv;                         // features and the FeatureVector in CSR form (fv_host.h)
    int nLeft, nUn;                  // KeyFrame::NLeft, mvKeysUn.size()
    unsigned desc, hasPoint, angles; // n x 32, uint8[n], float[n] (angles only with checkOrientation; 0 = not staged)
};
// ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (src/ORBmatcher.cc:864-1004; kernels_bow_kf.hip) for keyframe 1 against every
// neighbour of a call.  One arena as above.
struct FtBowKfJob {  // one neighbour
    FtBowArenaSide K2;
    unsigned matches;  // int[K1.n], -1 from the host's fill
    unsigned claimed;  // int[K2.n], 0 from the host's fill: vbMatched2 of the lists too long for the registers
};
struct FtBowKfCall {
    uint8_t *arena;
    FtBowArenaSide K1;
    unsigned jobs;      // FtBowKfJob[nNeighbours]
    unsigned nMatches;  // int[nNeighbours]
    int nNeighbours, checkOrientation;
    float nnRatio;
};
// the two launches of a call, in this order
int ft_launch_bow_kf_match(hipStream_t st, const FtBowKfCall &T);
int ft_launch_bow_kf_finish(hipStream_t st, const FtBowKfCall &T);

// ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (src/ORBmatcher.cc:322-524; kernels_bow_cand.hip) for one frame against every
// candidate keyframe of a call (Tracking::Relocalization, src/Tracking.cc:3839-3860).  One arena as above; the frame's descriptors
// alone are a pointer, because they may be read where a front end left them.
struct FtBowCandJob {  // one candidate keyframe
    FtBowArenaSide K;
    unsigned matches;  // int[F.n], -1 from the host's fill: the job's row, which also carries its claims
};
struct FtBowCandCall {
    uint8_t *arena;
    const uint8_t *frameDesc;  // F.n x 32: arena + F.desc, or the caller's device pointer
    FtBowArenaSide F;          // (the frame has no hasPoint)
    unsigned jobs;      // FtBowCandJob[nCandidates]
    unsigned nMatches;  // int[nCandidates]
    int nCandidates, maxNodes;  // maxNodes: the largest K.nNodes of the call (the grid's x extent in waves)
    int nLeft, checkOrientation;
    float nnRatio;
};
// the two launches of a call, in this order
int ft_launch_bow_cand_match(hipStream_t st, const FtBowCandCall &T);
int ft_launch_bow_cand_finish(hipStream_t st, const FtBowCandCall &T);

// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:329-403; kernels_distinct.hip) for every map point of a call.  One arena
// as above.  The host bins the points with a non-empty list by list length into four job lists, one behind the other in `jobs`:
// N <= 8, N <= 16 (both served by k_distinct_short), N <= 64 (k_distinct_wave), N <= FT_DISTINCT_MAX_OBSERVATIONS
// (k_distinct_block).  A job is the point's index; its list is descriptor rows [offsets[p], offsets[p + 1]).
struct FtDistinctCall {
    uint8_t *arena;
    unsigned offsets;     // int[nPoints + 1]: obs_offsets
    unsigned desc;        // offsets[nPoints] x 32 bytes
    unsigned jobs;        // int[n8 + n16 + nWave + nBlock]
    unsigned bestIdx;     // int[nPoints], -1 from the host's fill
    unsigned bestMedian;  // int[nPoints], -1 from the host's fill
    unsigned outDesc;     // nPoints x 32 bytes; the rows of points with an empty list are never written
    int n8, n16, nWave, nBlock;
};
// the launches of a call; a class without a job is not launched
int ft_launch_distinct_short(hipStream_t st, const FtDistinctCall &T);
int ft_launch_distinct_wave(hipStream_t st, const FtDistinctCall &T);
int ft_launch_distinct_block(hipStream_t st, const FtDistinctCall &T);

// KeyFrameDatabase::DetectNBestCandidates / DetectRelocalizationCandidates up to the scores (src/KeyFrameDatabase.cc:615-666,
// :741-787; kernels_kfdb.hip) for every stored keyframe of a database.  The BowVectors are resident: ids in one array, values in
// another, ROW r (a stored keyframe, in handle order) owns words [rowStart[r], rowStart[r] + rowLen[r]); an erased row has
// rowLen 0.  The per-keyframe members of the query's kind (mnPlaceRecognitionQuery / Words / Score, or the mnReloc* set) are
// one 16-byte record per row.  The call's arena: the call slot, the query and the connected rows go up; the slot, the records of
// the scored rows and their doubles come down; `first` stays on the device.
struct FtKfdbState {
    long long stamp;  // mn*Query
    int words;        // mn*Words
    float score;      // m*Score
};
struct FtKfdbRec {  // a scored row, in the order the waves finished (the host orders them by (first, row))
    int row, first, words;
    float score;
};
struct FtKfdbCall {
    const unsigned *ids;       // stored word ids
    const double *vals;        // stored word values
    const unsigned *rowStart;  // [nRows]
    const int *rowLen;         // [nRows]
    FtKfdbState *state;        // [nRows], of the query's kind
    int nRows;
    uint8_t *arena;
    unsigned slot;       // int[16]: [0] listed rows, [1] maxCommonWords, [2] scored rows; zero from the host
    unsigned qIds;       // unsigned[nQuery] strictly ascending
    unsigned qVals;      // double[nQuery]
    unsigned connected;  // int[nConnected] rows, ascending
    unsigned recs;       // FtKfdbRec[nRows]
    unsigned raw;        // double[nRows]: the score before the rounding to float, beside recs
    unsigned first;      // unsigned[nRows]: a listed row's first shared word, FT_KFDB_NOT_LISTED otherwise
    int nQuery, nConnected;
    long long queryId;
};
#define FT_KFDB_NOT_LISTED 0xffffffffu
int ft_launch_kfdb_count(hipStream_t st, const FtKfdbCall &T);
int ft_launch_kfdb_score(hipStream_t st, const FtKfdbCall &T);
// rows of a database into new storage (growth, compaction): new row r takes the words of old row map[r]
int ft_launch_kfdb_move(hipStream_t st, const unsigned *oldIds, const double *oldVals, const unsigned *oldStart, const int *map,
                        unsigned *newIds, double *newVals, const unsigned *newStart, const int *newLen, int nRows);

// ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) and Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1247-1437,
// :1439-1554; kernels_fuse.hip) for one list of map points against every target of a call.  A TARGET is one (keyframe, camera):
// the host hands the searched camera's keypoints over as a one-camera device frame (F.Nleft == -1; the right camera of a
// two-camera keyframe with its own keys, descriptor rows and mpCamera2 in F.cam), so that the grid and the window scan are those of
// any frame; idxOffset (NLeft for bRight) turns a keypoint of that frame back into the keyframe's index.  Every pointer of a
// record points into the call's device arena (the kernels re-derive them from it: FramePtrs, search_dev.h).
struct FtFuseTarget {
    FtDevFrame F;          // with its grid: gridStart[0] / gridRec[0] / gridDesc[0], filled by k_fuse_grid
    FtPose Tcw;            // Sophus form (quat != 0)
    float Ow[3];
    float logScaleFactor, th;
    float invSigma2[FT_MAX_LEVELS];  // mvInvLevelSigma2, read when checkReproj
    int checkReproj;       // the chi-square test of the SE3 overload (:1371-1395)
    int idxOffset;
    const uint8_t *valid;  // [M] or null: all
    int *bestIdx, *bestDist;  // [M] each
    uint8_t *stage;        // [M] or null
    int *nFound;           // [1], zero on entry
};
struct FtFusePoints {
    int M;
    const float *worldPos, *normal, *maxDist, *minDist;
    const uint8_t *desc;
};
// exit codes of a point (include/fasttrack_amd.h, ft_fuse_search)
#define FT_FUSE_SEARCHED 0
#define FT_FUSE_SKIPPED 1
#define FT_FUSE_DEPTH 2
#define FT_FUSE_IMAGE 3
#define FT_FUSE_DISTANCE 4
#define FT_FUSE_NORMAL 5
#define FT_FUSE_EMPTY 6
// the two launches of a call, in this order; arena: the call's device arena, targets: its FtFuseTarget[nTargets]
int ft_launch_fuse_grid(hipStream_t st, void *arena, const FtFuseTarget *targets, int nTargets, int maxLevels);
int ft_launch_fuse_search(hipStream_t st, void *arena, const FtFuseTarget *targets, int nTargets, const FtFusePoints &P);

// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) and its overload with vpPointsKFs / vpMatchedKF
// (src/ORBmatcher.cc:526-631, :633-745; kernels_sim3.hip) for n_jobs independent searches against ONE keyframe.  A JOB is one call
// of the reference: its own point list, pose, radius, threshold, projection form and vpMatched.  The keyframe's left camera is a
// one-camera device frame (F.Nleft == -1, as a Fuse target) handed to the kernels as an argument; every pointer of a job record
// points into the call's device arena (Rebase).  A candidate is a make_key key of a keypoint that was free on entry, lies in the
// band [level - 1, level] of the point's window and is no farther than the job's threshold: per point the FT_SIM3_TOP smallest
// (ascending) and their number.  The resolution scans a point's window again in the rare case that all of its top record is
// taken and the window holds more, so no list has a capacity.
#define FT_SIM3_TOP 4
#define FT_SIM3_NOWRITE 7  // stage: the window held keypoints and the point wrote nothing (0 = it wrote)
struct FtSim3Proj {
    float u, v, radius;
    int level;
};
struct FtSim3Job {
    FtFusePoints P;
    const uint8_t *valid;  // [P.M] or null: all
    FtPose Tcw;            // Sophus form (quat != 0)
    float Ow[3];
    float logScaleFactor, th;
    int thr;          // the largest distance d with (float)d <= TH_LOW * ratioHamming
    int handPinhole;  // the projection written out by hand (:672-677) instead of mpCamera->project (:564)
    int wantStage;    // the caller reads stage: tell an empty window (6) from an empty band
    int *matched;        // [F.N] in / out: -1 = NULL
    int *pointKeypoint;  // [M]
    uint8_t *stage;      // [M]
    int *nMatches;       // [1]
    FtSim3Proj *proj;         // [M] device only from here on
    unsigned long long *top;  // [M][FT_SIM3_TOP]
    int *count;               // [M] candidates of a point
    int *walk;                // [M] the points with candidates, in index order
};
// the three launches of a call, in this order; arena: the call's device arena, jobs: its FtSim3Job[nJobs]
int ft_launch_sim3_grid(hipStream_t st, const FtDevFrame &F);
int ft_launch_sim3_candidates(hipStream_t st, const FtDevFrame &F, void *arena, const FtSim3Job *jobs, int nJobs, int maxM);
int ft_launch_sim3_resolve(hipStream_t st, const FtDevFrame &F, void *arena, const FtSim3Job *jobs, int nJobs);
// dynamic LDS of the resolution: a taken bit per keypoint (<= FT_INIT_MAX_LDS: 1 228 800 keypoints)
inline size_t ft_sim3_lds_bytes(int nKeys) { return 4 * (((size_t)nKeys + 31) / 32); }

// Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:814-1114; kernels_pose_opt.hip) for every frame of a call: one workgroup
// per job, one launch.  One arena as above.  The host gathers a frame's correspondences in keypoint order into edge records
// (pose_opt.cpp); frames with fewer than three are answered by the host and have no job.
struct FtPoseEdge {
    float X[3];    // GetWorldPos()
    float obs[3];  // kpUn.pt.x, kpUn.pt.y, mvuRight (stereo)
    float w;       // mvInvLevelSigma2[kpUn.octave]
    int kind;      // 0 EdgeSE3ProjectXYZOnlyPose (pCamera), 1 ...ToBody (pCamera2, Trl), 2 EdgeStereoSE3ProjectXYZOnlyPose
};
struct FtPoseOptJob {
    unsigned edges;  // FtPoseEdge[nE]
    unsigned work;   // device only: float chi2[nE] (what the last computeError left, as the classification reads it), then uint8 level[nE]
    unsigned out;    // FtPoseOptOut
    unsigned flags;  // uint8[nE]: mvbOutlier of the edges
    int nE, model, twoCam;  // twoCam: the frame has to-body edges (Nleft != -1): trlQ / trlT are read
    float cam[8], cam2[8], bf;
    float q[4], t[3], trlQ[4], trlT[3];
};
struct FtPoseOptOut {
    float q[4], t[3];
    int ret;
    int iterations[4], rejected[4];
    double chi[4];
};
struct FtPoseOptCall {
    uint8_t *arena;
    unsigned jobs;  // FtPoseOptJob[nJobs]
    int nJobs;
};
int ft_launch_pose_opt(hipStream_t st, const FtPoseOptCall &T);

// Sim3Solver (src/Sim3Solver.cc; kernels_sim3_solver.hip) for every problem of a call: three launches whatever the problems hold - a
// lane per (job, iteration) computes the hypothesis, a wave per (job, iteration) counts its inliers, a workgroup per job selects.
// One arena as above.  The host gathers the valid pairs of a problem in index order into records (sim3_solver.cpp); a problem with
// fewer pairs than min_inliers is answered by the host and has no job.
struct FtSim3Pair {
    float X1[3], max1;  // mvX3Dc1, mvnMaxError1
    float X2[3], max2;  // mvX3Dc2, mvnMaxError2
    float P1[2], P2[2];  // mvP1im1, mvP2im2
};
struct FtSim3Hyp {
    float T12[12], T21[12];  // mT12i, mT21i: the rows [sR | t] of the upper 3 x 4
    float R[9], s;           // mR12i, ms12i
    float pad[2];
};
struct FtSim3SolverJob {
    unsigned pairs;   // FtSim3Pair[N]
    unsigned draws;   // int[3 * eff]: rand() of the iterations
    unsigned hyps;    // device only: FtSim3Hyp[eff]
    unsigned counts;  // int[eff]: mnInliersi
    unsigned out;     // FtSim3SolverOut
    unsigned flags;   // uint8[N]: mvbBestInliers
    int N, eff, minInliers, fixScale, model1, model2;  // eff: mRansacMaxIts as SetRansacParameters leaves it
    float cam1[8], cam2[8];
};
struct FtSim3SolverOut {
    int converged, iterations, nBest, best;  // best: the iteration (from 0) whose hypothesis is mBest*
    FtSim3Hyp hyp;
};
struct FtSim3SolverCall {
    uint8_t *arena;
    unsigned jobs;  // FtSim3SolverJob[nJobs]
    int nJobs, maxEff;
};
int ft_launch_sim3_hypotheses(hipStream_t st, const FtSim3SolverCall &T);
int ft_launch_sim3_count(hipStream_t st, const FtSim3SolverCall &T);
int ft_launch_sim3_select(hipStream_t st, const FtSim3SolverCall &T);

#ifdef __HIPCC__
// rotation bin of a match (src/ORBmatcher.cc:817-823, 2171-2176): float arithmetic, round() half away from zero; host twin of the pair: rot_hist.h,
// the filter of a workgroup over them: rot_filter_dev.h
__device__ __forceinline__ int init_bin(float angle1, float angle2) {
    float rot = __fsub_rn(angle1, angle2);
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    int bin = (int)roundf(__fmul_rn(rot, 1.0f / FT_HISTO_LENGTH));
    if (bin == FT_HISTO_LENGTH) bin = 0;
    return bin;
}
// ComputeThreeMaxima (src/ORBmatcher.cc:2210-2251) on the bin sizes: bit b of the result = bin b is kept
__device__ __forceinline__ int three_maxima_keep(const int *hist) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int b = 0; b < FT_HISTO_LENGTH; b++) {
        const int sz = hist[b];
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
    if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) { ind3 = -1; }
    int keep = 0;
    if (ind1 >= 0) keep |= 1 << ind1;
    if (ind2 >= 0) keep |= 1 << ind2;
    if (ind3 >= 0) keep |= 1 << ind3;
    return keep;
}
struct Window {
    int minCX, maxCX, minCY, maxCY;
    bool empty;
};

// Frame::GetFeaturesInArea cell window (src/Frame.cc:689-711)
__device__ __forceinline__ Window cell_window(const FtDevFrame &F, float x, float y, float r) {
    Window w;
    w.empty = false;
    w.minCX = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, F.mnMinX), r), F.invW)));
    if (w.minCX >= FT_GRID_COLS) w.empty = true;
    w.maxCX = min(FT_GRID_COLS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, F.mnMinX), r), F.invW)));
    if (w.maxCX < 0) w.empty = true;
    w.minCY = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, F.mnMinY), r), F.invH)));
    if (w.minCY >= FT_GRID_ROWS) w.empty = true;
    w.maxCY = min(FT_GRID_ROWS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, F.mnMinY), r), F.invH)));
    if (w.maxCY < 0) w.empty = true;
    return w;
}

// what a record's byte offset names in the arena of its call
template <class T>
__device__ __forceinline__ const T *at(const uint8_t *arena, unsigned off) {
    return (const T *)(arena + off);
}
// the entry of `node` in the ascending node ids of a FeatureVector (the reference's lower_bound walk over two FeatureVectors
// visits exactly the common keys), or -1
__device__ __forceinline__ int fv_find_node(const unsigned *nodes, int nNodes, unsigned node) {
    int lo = 0, hi = nNodes;  // lower_bound
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (nodes[mid] < node) lo = mid + 1;
        else hi = mid;
    }
    return lo < nNodes && nodes[lo] == node ? lo : -1;
}

// Re-derives a pointer read from a job record from the arena pointer the kernel got as an argument (FramePtrs, search_dev.h: a
// pointer out of memory is a generic pointer to the compiler): arena + (p - address of the arena, passed as an integer)
struct Rebase {
    uint8_t *arena;
    unsigned long long addr;  // (unsigned long long)arena
    template <class T>
    __device__ __forceinline__ T *operator()(T *p) const {
        return p ? (T *)(arena + ((unsigned long long)p - addr)) : nullptr;
    }
};
// (host: what every launch of a batch passes for its arena)
inline Rebase rebase_of(void *arena) { return Rebase{(uint8_t *)arena, (unsigned long long)(uintptr_t)arena}; }
// (host) A kernel that takes up to FT_INIT_MAX_LDS of dynamic LDS, more than the default 64 KB, is told so once per device, in
// front of its launch; the table of the devices that know is the instantiation's, one per kernel.
template <auto Kernel>
inline int ft_allow_max_lds() {
    static int ldsSet[64];
    int dev = 0;
    FT_HIP(hipGetDevice(&dev));
    if (dev >= 0 && dev < 64 && !__atomic_load_n(&ldsSet[dev], __ATOMIC_ACQUIRE)) {
        FT_HIP(hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FT_INIT_MAX_LDS));
        __atomic_store_n(&ldsSet[dev], 1, __ATOMIC_RELEASE);
    }
    return FT_OK;
}
#endif

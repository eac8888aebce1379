// HIP kernels of the map-point fusion search for gfx950 (wave64):
//   ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint *> &vpMapPoints, th, bRight)            (reference src/ORBmatcher.cc:1247-1437)
//   ORBmatcher::Fuse(KeyFrame *pKF, Sophus::Sim3f &Scw, vpPoints, th, vpReplacePoint)             (:1439-1554)
//
// For every point the reference projects into the keyframe, tests depth, image, distance range and viewing angle, predicts the
// level, takes KeyFrame::GetFeaturesInArea (no level filter) and keeps, among the keypoints of octave level - 1 .. level that pass
// the chi-square test of the reprojection error (SE3 overload only), the nearest descriptor - the first of equal distances in
// GetFeaturesInArea's order.  None of that depends on what the bookkeeping behind the loop (Replace, AddObservation, AddMapPoint)
// changes inside the call: it only decides which LATER points are skipped at the top of the loop, which the caller re-tests when it
// applies the results in order.  So a (target, point) pair is independent of every other one:
//   k_fuse_grid    the per-octave grid (build_grid_body, search_dev.h) of every target's keypoints, workgroup (octave, target)
//   k_fuse_search  a ROW of 16 lanes per (target, point), four points per wave: the tests of :1297-1343 (every lane of the row
//                  computes them), then the window in the grid with the level band as the scan's octave range
//                  (row_for_window, search_dev.h), the chi-square test, the Hamming distance; the row minimum of the key
//                  (distance, cell x, cell y, index) is the reference's strict `dist < bestDist` over GetFeaturesInArea's order.
// Two launches per call, whatever the number of targets and points.  blockIdx.y is the target: everything a workgroup reads of
// it sits at a uniform address (scalar loads).
#include <algorithm>

#include "search_dev.h"

namespace {

__global__ __launch_bounds__(256) void k_fuse_grid(const FtFuseTarget *__restrict__ targets, Rebase rb) {
    const FtDevFrame &F = targets[blockIdx.y].F;
    if ((int)blockIdx.x >= F.nlevels) return;
    const FramePtrs Q = frame_ptrs(F, rb);
    build_grid_body(F, Q, blockIdx.x, 0, (int *)Q.gridStart[0], nullptr, (float4 *)Q.gridRec[0], (uint8_t *)Q.gridDesc[0], nullptr, nullptr);
}

// what the tests in front of the window leave of a point
struct FusePoint {
    int stage;  // FT_FUSE_* (FT_FUSE_SEARCHED: the window is to be scanned)
    int level;
    float u, v, ur, radius;
};

// :1278-1343 (:1461-1503) for point i of target T
__device__ __forceinline__ FusePoint fuse_point(const FtFuseTarget &T, const uint8_t *valid, const FtFusePoints &P, int i) {
    const FtDevFrame &F = T.F;
    FusePoint r;
    r.stage = FT_FUSE_SKIPPED;
    r.level = 0;
    r.u = r.v = r.ur = r.radius = 0.f;
    if (valid && !valid[i]) return r;  // !pMP, isBad(), IsInKeyFrame(pKF) / spAlreadyFound.count(pMP)
    const float xw[3] = {P.worldPos[3 * i], P.worldPos[3 * i + 1], P.worldPos[3 * i + 2]};
    float xc[3], uv[2];
    transform_pose(T.Tcw.m, T.Tcw.q, 1, xw, xc);
    r.stage = FT_FUSE_DEPTH;
    if (xc[2] < 0.0f) return r;  // (+-0 pass: invz is what IEEE makes of it)
    const float invz = __fdiv_rn(1.0f, xc[2]);
    project_cam(F, xc, uv);
    r.stage = FT_FUSE_IMAGE;
    // KeyFrame::IsInImage (src/KeyFrame.cc:750-753): a NaN fails it
    if (!(uv[0] >= F.mnMinX && uv[0] < F.mnMaxX && uv[1] >= F.mnMinY && uv[1] < F.mnMaxY)) return r;
    const float PO[3] = {__fsub_rn(xw[0], T.Ow[0]), __fsub_rn(xw[1], T.Ow[1]), __fsub_rn(xw[2], T.Ow[2])};
    const float dist3D = norm3(PO);
    const float maxRaw = P.maxDist[i];
    const float maxDistance = __fmul_rn(1.2f, maxRaw), minDistance = __fmul_rn(0.8f, P.minDist[i]);
    r.stage = FT_FUSE_DISTANCE;
    if (dist3D < minDistance || dist3D > maxDistance) return r;
    const float Pn[3] = {P.normal[3 * i], P.normal[3 * i + 1], P.normal[3 * i + 2]};
    r.stage = FT_FUSE_NORMAL;
    if ((double)dot3(PO, Pn) < 0.5 * (double)dist3D) return r;  // `PO.dot(Pn)<0.5*dist3D`: the float dot against a double product
    r.stage = FT_FUSE_SEARCHED;
    r.level = predict_scale(maxRaw, dist3D, T.logScaleFactor, F.nlevels);
    r.u = uv[0];
    r.v = uv[1];
    r.ur = __fsub_rn(uv[0], __fmul_rn(F.mbf, invz));
    r.radius = __fmul_rn(T.th, F.sf[r.level]);
    return r;
}

// the chi-square test of the reprojection error (:1371-1395) for a keypoint of the band; inv = mvInvLevelSigma2[its octave]
__device__ __forceinline__ bool fuse_reprojects(const FusePoint &p, const WinEntry &kp, float inv) {
    const float ex = __fsub_rn(p.u, kp.x), ey = __fsub_rn(p.v, kp.y);
    const float exy = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
    if (kp.uright >= 0.f) {
        const float er = __fsub_rn(p.ur, kp.uright);
        const float e2 = __fadd_rn(exy, __fmul_rn(er, er));
        return !((double)__fmul_rn(e2, inv) > 7.8);  // (a float product against the double constant)
    }
    return !((double)__fmul_rn(exy, inv) > 5.99);
}

__device__ __forceinline__ void fuse_store(const FtFuseTarget &T, const Rebase &rb, int i, int stage, unsigned long long best) {
    const int bd = best == KEY_NONE ? 256 : key_dist(best);
    rb(T.bestIdx)[i] = best == KEY_NONE ? -1 : key_idx(best) + T.idxOffset;
    rb(T.bestDist)[i] = bd;
    uint8_t *st = rb(T.stage);
    if (st) st[i] = (uint8_t)stage;
    if (bd <= FT_TH_LOW) atomicAdd(rb(T.nFound), 1);
}

#define FT_FUSE_PPB 16  // points per workgroup: 4 waves x 4 rows
__global__ __launch_bounds__(256) void k_fuse_search(const FtFuseTarget *__restrict__ targets, Rebase rb, FtFusePoints P) {
    __shared__ unsigned rowLists[FT_FUSE_PPB][FT_ROW_LIST];
    unsigned *list = rowLists[threadIdx.x >> 4];
    const int lane = threadIdx.x & 63, sub = lane & 15, rowBase = lane & 48;
    const int i = (int)blockIdx.x * FT_FUSE_PPB + (int)(threadIdx.x >> 4);
    if (i >= P.M) return;
    const FtFuseTarget &T = targets[blockIdx.y];
    const FtDevFrame &F = T.F;
    const FramePtrs Q = frame_ptrs(F, rb);
    const FusePoint p = fuse_point(T, rb(T.valid), P, i);
    int stage = p.stage;
    unsigned long long k0 = KEY_NONE;
    if (stage == FT_FUSE_SEARCHED) {
        const Window w = cell_window(F, p.u, p.v, p.radius);
        bool any = false;
        if (!w.empty) {
            unsigned long long q[4];
            load_desc256(P.desc, i, q);
            const int level = p.level, check = T.checkReproj;
            const float invLo = T.invSigma2[max(level - 1, 0)], invHi = T.invSigma2[level];
            // the band [level - 1, level] (:1368) is the scan's octave range: what reaches the visitor passed band and box
            row_for_window(F, Q, 0, w, level - 1, level, p.u, p.v, p.radius, sub, rowBase, list, [&](const WinEntry &kp, bool real) {
                any = any || real;
                bool cand = real;
                if (cand && check) cand = fuse_reprojects(p, kp, kp.octave == level ? invHi : invLo);
                const unsigned long long key = make_key(hamming256(q, kp.d), kp.cx, kp.cy, kp.idx, kp.octave, false);
                if (cand) k0 = key < k0 ? key : k0;
            });
            any = ((unsigned)(__ballot(any) >> rowBase) & 0xffffu) != 0u;
            // `if(vIndices.empty())` (:1347) looks at every octave: only the exit code depends on it when the band is empty
            if (!any && T.stage) {
                row_for_window(F, Q, 0, w, -1, -1, p.u, p.v, p.radius, sub, rowBase, list, [&](const WinEntry &, bool real) { any = any || real; });
                any = ((unsigned)(__ballot(any) >> rowBase) & 0xffffu) != 0u;
            }
        }
        if (!any) stage = FT_FUSE_EMPTY;
        k0 = row_min_u64(k0);
    }
    if (sub == 0) fuse_store(T, rb, i, stage, k0);
}

}  // namespace

int ft_launch_fuse_grid(hipStream_t st, void *arena, const FtFuseTarget *targets, int nTargets, int maxLevels) {
    hipLaunchKernelGGL(k_fuse_grid, dim3(maxLevels, nTargets), dim3(256), 0, st, targets, rebase_of(arena));
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_fuse_search(hipStream_t st, void *arena, const FtFuseTarget *targets, int nTargets, const FtFusePoints &P) {
    hipLaunchKernelGGL(k_fuse_search, dim3((P.M + FT_FUSE_PPB - 1) / FT_FUSE_PPB, nTargets), dim3(256), 0, st, targets, rebase_of(arena), P);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

// HIP kernels of ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, vpMapPointMatches) (reference src/ORBmatcher.cc:322-524) for
// gfx950 (wave64): one frame against every candidate keyframe of a call (the loop of Tracking::Relocalization,
// src/Tracking.cc:3839-3860), two launches whatever the number of candidates.
//   k_bow_cand_match   blockIdx.y = candidate.  The unit of work is one (candidate, node of that candidate) pair, a WAVE per unit,
//                      and the unit's body is k_search_by_bow's walk (bow_walk_node, bow_walk_dev.h) against the job table: binary
//                      search for the node on the frame's side, a frame node of up to 256 features in registers, the candidate's
//                      features of the node 64 at a time and one per step by v_readlane; a longer frame node through memory, its
//                      claims in the job's own row of `matches`, written and read back by the same lane.  The frame side is staged
//                      once and read by the waves of every candidate.  A unit writes row k only, and only the entries of the frame
//                      features of its node: neither the nodes of a candidate nor the candidates of a call share anything.
//   k_bow_cand_finish  a workgroup per candidate: rotation histogram of kf angle - frame angle over the row (:489-497),
//                      ComputeThreeMaxima, the removal (:500-521), nmatches.  Without checkOrientation it only counts.
// Why blockIdx.y and not a flat unit list.  A flat list is one more array of n_keyframes x nodes records that the host builds and
// the call uploads, to spare the waves beyond a candidate's own node count - which return on one scalar compare; the candidates
// of a relocalisation are keyframes of the same map and vocabulary level, so their node counts are close and few such waves exist.
// The grid's y extent bounds a call at 65 535 candidates, as k_bow_kf_match bounds ft_search_by_bow_keyframes.
#include <algorithm>

#include "bow_walk_dev.h"
#include "ft_internal.h"
#include "ft_search.h"
#include "rot_filter_dev.h"
#include "wave_ops.h"

namespace {

#define FT_BOWCAND_FIN_T 256

__global__ __launch_bounds__(256) void k_bow_cand_match(FtBowCandCall T) {
    const uint8_t *arena = T.arena;
    const int lane = threadIdx.x & 63;
    const int a = (int)blockIdx.x * 4 + wave_index();
    const FtBowCandJob *job = at<FtBowCandJob>(arena, T.jobs) + blockIdx.y;
    const int n = job->K.fv.n, nNodes = job->K.fv.nNodes;
    if (a >= nNodes || n <= 0) return;  // nothing of an empty candidate is dereferenced
    const FtBowSide K{n, nNodes, at<unsigned>(arena, job->K.fv.nodes), at<int>(arena, job->K.fv.offsets), at<unsigned>(arena, job->K.fv.feats),
                      arena + job->K.desc};
    const FtBowSide F{T.F.fv.n, T.F.fv.nNodes, at<unsigned>(arena, T.F.fv.nodes), at<int>(arena, T.F.fv.offsets), at<unsigned>(arena, T.F.fv.feats),
                      T.frameDesc};
    bow_walk_node(K, arena + job->K.hasPoint, F, T.nLeft, T.nnRatio, (int *)(T.arena + job->matches), a, lane);
}

__global__ __launch_bounds__(FT_BOWCAND_FIN_T) void k_bow_cand_finish(FtBowCandCall T) {
    uint8_t *arena = T.arena;
    const FtBowCandJob *job = at<FtBowCandJob>(arena, T.jobs) + blockIdx.x;
    const float *angleKf = at<float>(arena, job->K.angles), *angleF = at<float>(arena, T.F.angles);
    // kp.angle - Fkp.angle (:491): the keyframe's minus the frame's, and the row is the frame's; the removal :509-519
    rot_filter_rows<FT_BOWCAND_FIN_T>((int *)(arena + job->matches), T.F.fv.n, T.checkOrientation, (int *)(arena + T.nMatches) + blockIdx.x,
                                      [&](int i, int m) { return init_bin(angleKf[m], angleF[i]); });
}

}  // namespace

int ft_launch_bow_cand_match(hipStream_t st, const FtBowCandCall &T) {
    const dim3 grid((unsigned)std::max((T.maxNodes + 3) / 4, 1), (unsigned)T.nCandidates);
    hipLaunchKernelGGL(k_bow_cand_match, grid, dim3(256), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_bow_cand_finish(hipStream_t st, const FtBowCandCall &T) {
    hipLaunchKernelGGL(k_bow_cand_finish, dim3((unsigned)T.nCandidates), dim3(FT_BOWCAND_FIN_T), 0, st, T);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

// Sim3Solver (src/Sim3Solver.cc) for every problem of a call: ft_sim3_solver.  The host checks the problems, gathers the valid pairs of
// each in index order into 48-byte records (the constructor, :35-121: mvX3Dc1 / mvX3Dc2, mvnMaxError1 / 2, mvP1im1 / mvP2im2 - the
// projections are made HERE, with the text of the device's project) and computes the iteration count of SetRansacParameters
// (:123-147) - straight into the pinned mirror of the arena.  Then one block up (jobs, pairs, draws), THREE launches
// (kernels_sim3_solver.hip: the hypotheses, their inlier counts, the selection), the results down, one wait.  A problem with fewer
// pairs than min_inliers is answered here (:225-229) and has no job.  Nothing of the sequence depends on the number of problems.
#include <cmath>

#include "search_host.h"
// (behind the HIP runtime, whose qualifiers it uses)
#include "libm_f32.h"

namespace {

const char *const FN = "ft_sim3_solver";

inline float sum3(float e0, float e1, float e2) { return e0 + (e1 + e2); }  // Eigen's association (redux_novec_unroller)

// pCamera->project(Eigen::Vector3f) (Pinhole.cpp:43-49, KannalaBrandt8.cpp:67-84): the text of project() of kernels_sim3_solver.hip
// (this unit is compiled without contraction; sqrtf is correctly rounded, the other functions are libm_f32.h's on both sides)
void projectHost(int model, const float *cam, const float p[3], float uv[2]) {
    if (model == 0) {
        uv[0] = cam[0] * p[0] / p[2] + cam[2];
        uv[1] = cam[1] * p[1] / p[2] + cam[3];
        return;
    }
    const float x2y2 = p[0] * p[0] + p[1] * p[1];
    const float theta = ft_libm::atan2f_glibc(sqrtf(x2y2), p[2]);
    const float psi = ft_libm::atan2f_glibc(p[1], p[0]);
    const float t2 = theta * theta, t3 = theta * t2, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
    const float r = (((theta + cam[4] * t3) + cam[5] * t5) + cam[6] * t7) + cam[7] * t9;
    uv[0] = cam[0] * r * ft_libm::cosf_glibc(psi) + cam[2];
    uv[1] = cam[1] * r * ft_libm::sinf_glibc(psi) + cam[3];
}

// GetRotation() of a pose held as Sophus::SE3f: Quaternionf::toRotationMatrix(), row-major
void rotationOf(const float q[4], float R[9]) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1.f - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
    R[3] = txy + twz, R[4] = 1.f - (txx + tzz), R[5] = tyz - twx;
    R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.f - (txx + tyy);
}

// mRansacMaxIts as SetRansacParameters (:123-147) leaves it for N >= minInliers pairs.  The reference narrows the quotient to int
// before the min, which is undefined when epsilon is tiny: the min is taken in double, an infinite or NaN quotient counts as more
// than maxIts.
int effectiveIterations(double probability, int minInliers, int N, int maxIts) {
    if (minInliers == N) return 1;
    const float epsilon = (float)minInliers / N;
    const double q = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
    const int n = (std::isfinite(q) && q < (double)maxIts) ? (int)q : maxIts;
    return std::max(1, n);
}

int checkProblem(const std::string &w, const ft_sim3_problem *P, int *nPairs) {
    FT_REQUIRE(P->n >= 0 && P->n < (1 << 16), w + "n out of range");
    FT_REQUIRE(P->n == 0 || (P->valid && P->world_pos1 && P->world_pos2 && P->sigma2_1 && P->sigma2_2), w + "a pair array is null");
    FT_REQUIRE((P->cam_model1 == 0 || P->cam_model1 == 1) && (P->cam_model2 == 0 || P->cam_model2 == 1), w + "unknown camera model");
    FT_REQUIRE(P->probability > 0.0 && P->probability < 1.0, w + "probability outside (0, 1)");
    FT_REQUIRE(P->min_inliers >= 0, w + "min_inliers < 0");
    FT_REQUIRE(P->max_iterations >= 1, w + "max_iterations < 1");
    if (P->max_iterations > FT_SIM3_MAX_ITERATIONS) {
        ft_set_error(w + "max_iterations " + std::to_string(P->max_iterations) + " is beyond FT_SIM3_MAX_ITERATIONS");
        return FT_ERR_CAPACITY;
    }
    FT_REQUIRE(P->rand_draws, w + "rand_draws is null");
    for (int i = 0; i < 3 * P->max_iterations; i++)
        FT_REQUIRE(P->rand_draws[i] >= 0 && (long long)P->rand_draws[i] <= (long long)FT_SIM3_RAND_MAX, w + "a draw outside [0, RAND_MAX]");
    FtPose p;
    int rc = poseOfSe3(&P->Tcw1, p);
    if (rc == FT_OK) rc = poseOfSe3(&P->Tcw2, p);
    if (rc != FT_OK) {
        ft_set_error(w + "Tcw1.q / Tcw2.q is not a unit quaternion (x, y, z, w)");
        return rc;
    }
    int n = 0;
    for (int i = 0; i < P->n; i++) n += P->valid[i] ? 1 : 0;
    FT_REQUIRE(n < P->min_inliers || n >= 3, w + "fewer than three pairs with min_inliers not above them: no sample can be drawn");
    *nPairs = n;
    return FT_OK;
}

// :93-118 for the valid pairs of P, in index order
void gatherPairs(const ft_sim3_problem *P, FtSim3Pair *E) {
    float R1[9], R2[9];
    rotationOf(P->Tcw1.q, R1);
    rotationOf(P->Tcw2.q, R2);
    for (int i = 0; i < P->n; i++) {
        if (!P->valid[i]) continue;
        const float *X1 = P->world_pos1 + 3 * (size_t)i, *X2 = P->world_pos2 + 3 * (size_t)i;
        for (int k = 0; k < 3; k++) {  // Rcw * X3Dw + tcw
            E->X1[k] = sum3(R1[3 * k] * X1[0], R1[3 * k + 1] * X1[1], R1[3 * k + 2] * X1[2]) + P->Tcw1.t[k];
            E->X2[k] = sum3(R2[3 * k] * X2[0], R2[3 * k + 1] * X2[1], R2[3 * k + 2] * X2[2]) + P->Tcw2.t[k];
        }
        E->max1 = (float)(9.210 * P->sigma2_1[i]);  // push_back of a double product into a vector<float>
        E->max2 = (float)(9.210 * P->sigma2_2[i]);
        projectHost(P->cam_model1, P->cam1, E->X1, E->P1);  // FromCameraToImage
        projectHost(P->cam_model2, P->cam2, E->X2, E->P2);
        E++;
    }
}

void identityResult(ft_sim3_result *r) {
    memset(r, 0, sizeof *r);
    r->no_more = 1;
    r->T12[0] = r->T12[5] = r->T12[10] = r->T12[15] = 1.f;
    r->R[0] = r->R[4] = r->R[8] = 1.f;
    r->s = 1.f;
}

}  // namespace

extern "C" int ft_sim3_solver(ft_context *ctx, int n_problems, const ft_sim3_problem *problems, ft_sim3_result *results, uint8_t *const *inliers,
                              uint8_t *const *best_inliers, int *const *hypothesis_inliers) {
    const std::string who = FN;
    FT_REQUIRE(ctx, who + ": null context");
    FT_REQUIRE(n_problems >= 0 && n_problems < (1 << 16), who + ": n_problems out of range");
    FT_REQUIRE(n_problems == 0 || (problems && results && inliers), who + ": null argument");
    std::vector<int> nP((size_t)n_problems), eff((size_t)n_problems, 0);
    int nJobs = 0, maxEff = 0;
    size_t totalPairs = 0, totalHyp = 0;
    for (int p = 0; p < n_problems; p++) {
        const ft_sim3_problem *P = problems + p;
        const std::string w = who + ": problem " + std::to_string(p) + ": ";
        const int rc = checkProblem(w, P, &nP[p]);
        if (rc != FT_OK) return rc;
        FT_REQUIRE(P->n == 0 || (inliers[p] && (!best_inliers || best_inliers[p])), w + "inliers or best_inliers is null");
        FT_REQUIRE(!hypothesis_inliers || hypothesis_inliers[p], w + "hypothesis_inliers is null");
        if (nP[p] < P->min_inliers) continue;
        eff[p] = effectiveIterations(P->probability, P->min_inliers, nP[p], P->max_iterations);
        nJobs++, totalPairs += (size_t)nP[p], totalHyp += (size_t)eff[p];
        maxEff = std::max(maxEff, eff[p]);
    }
    auto jobless = [&](int p) {  // :225-229
        identityResult(results + p);
        for (int i = 0; i < problems[p].n; i++) {
            inliers[p][i] = 0;
            if (best_inliers) best_inliers[p][i] = 0;
        }
    };
    if (nJobs == 0) {
        for (int p = 0; p < n_problems; p++) jobless(p);
        return FT_OK;
    }
    int rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    // the arena: jobs | pairs of all jobs | draws of all jobs || hypotheses (device only) | counts | results | best-inlier flags of the pairs
    Arena a;
    const size_t oJobs = a.take(sizeof(FtSim3SolverJob) * (size_t)nJobs);
    const size_t oPairs = a.take(sizeof(FtSim3Pair) * totalPairs);
    const size_t oDraws = a.take(sizeof(int) * 3 * totalHyp);
    const size_t inputEnd = a.off;
    const size_t oHyps = a.take(sizeof(FtSim3Hyp) * totalHyp);
    const size_t oCounts = a.take(sizeof(int) * totalHyp);
    const size_t oOut = a.take(sizeof(FtSim3SolverOut) * (size_t)nJobs);
    const size_t oFlags = a.take(totalPairs);
    if (a.off >= ((size_t)1 << 32)) {  // the jobs address the arena with 32-bit offsets
        ft_set_error(who + ": the arena of the call would pass 4 GB");
        return FT_ERR_CAPACITY;
    }
    rc = ft_ensure_scratch(ctx, a.off, a.off);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    FtSim3SolverJob *jobs = (FtSim3SolverJob *)(pin + oJobs);
    FtSim3Pair *pairs = (FtSim3Pair *)(pin + oPairs);
    int *draws = (int *)(pin + oDraws);
    size_t e0 = 0, h0 = 0;
    for (int p = 0, j = 0; p < n_problems; p++) {
        if (!eff[p]) continue;
        const ft_sim3_problem *P = problems + p;
        FtSim3SolverJob &J = jobs[j];
        memset(&J, 0, sizeof J);
        J.pairs = (unsigned)(oPairs + sizeof(FtSim3Pair) * e0);
        J.draws = (unsigned)(oDraws + sizeof(int) * 3 * h0);
        J.hyps = (unsigned)(oHyps + sizeof(FtSim3Hyp) * h0);
        J.counts = (unsigned)(oCounts + sizeof(int) * h0);
        J.out = (unsigned)(oOut + sizeof(FtSim3SolverOut) * (size_t)j);
        J.flags = (unsigned)(oFlags + e0);
        J.N = nP[p], J.eff = eff[p], J.minInliers = P->min_inliers, J.fixScale = P->fix_scale ? 1 : 0;
        J.model1 = P->cam_model1, J.model2 = P->cam_model2;
        memcpy(J.cam1, P->cam1, sizeof J.cam1);
        memcpy(J.cam2, P->cam2, sizeof J.cam2);
        gatherPairs(P, pairs + e0);
        memcpy(draws + 3 * h0, P->rand_draws, sizeof(int) * 3 * (size_t)eff[p]);
        e0 += (size_t)nP[p], h0 += (size_t)eff[p];
        j++;
    }
    FtSim3SolverCall T;
    T.arena = dev;
    T.jobs = (unsigned)oJobs;
    T.nJobs = nJobs;
    T.maxEff = maxEff;
    hipStream_t st = ctx->stream;
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, inputEnd);  // one copy: the block is contiguous
    C.launch("kernel.sim3_hypotheses", [&] { return ft_launch_sim3_hypotheses(st, T); });
    C.launch("kernel.sim3_count", [&] { return ft_launch_sim3_count(st, T); });
    C.launch("kernel.sim3_select", [&] { return ft_launch_sim3_select(st, T); });
    rc = C.down(oCounts, a.off);
    if (rc != FT_OK) return rc;
    e0 = h0 = 0;
    for (int p = 0, j = 0; p < n_problems; p++) {
        const ft_sim3_problem *P = problems + p;
        if (!eff[p]) {
            jobless(p);
            continue;
        }
        const FtSim3SolverOut *O = (const FtSim3SolverOut *)(pin + oOut) + j;
        const uint8_t *fl = pin + oFlags + e0;
        const bool conv = O->converged != 0;
        for (int i = 0, k = 0; i < P->n; i++) {  // vbInliers[mvnIndices1[i]] = true, only when converged (:277-279)
            const uint8_t b = P->valid[i] ? fl[k++] : 0;
            inliers[p][i] = conv ? b : 0;
            if (best_inliers) best_inliers[p][i] = b;
        }
        ft_sim3_result &r = results[p];
        memset(&r, 0, sizeof r);
        r.converged = conv ? 1 : 0;
        r.no_more = conv ? 0 : 1;  // :290: the run went through mRansacMaxIts iterations
        r.iterations = O->iterations;
        r.effective_iterations = eff[p];
        r.n_inliers = conv ? O->nBest : 0;
        r.n_best_inliers = O->nBest;
        r.best_iteration = O->best + 1;
        for (int i = 0; i < 12; i++) r.T12[i] = O->hyp.T12[i];
        r.T12[15] = 1.f;
        memcpy(r.R, O->hyp.R, sizeof r.R);
        for (int i = 0; i < 3; i++) r.t[i] = O->hyp.T12[4 * i + 3];
        r.s = O->hyp.s;
        if (hypothesis_inliers) memcpy(hypothesis_inliers[p], pin + oCounts + sizeof(int) * h0, sizeof(int) * (size_t)eff[p]);
        e0 += (size_t)nP[p], h0 += (size_t)eff[p];
        j++;
    }
    ctx->addStat("sim3_solver.total", tAll.ms());
    ctx->addStat("sim3_solver.launches", C.launches);
    return FT_OK;
}

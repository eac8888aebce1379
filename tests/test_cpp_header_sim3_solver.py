"""The C++ mirror of Sim3Solver (fasttrack::Sim3SolverBatch, include/fasttrack_amd.hpp) compiles with plain g++ and links against
the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <vector>
#include "fasttrack_amd.hpp"
// LoopClosing::DetectCommonRegionsFromBoW for the candidates of a keyframe: every solver of :698-710 in one call
int solveCandidates(fasttrack::Context &ctx, const std::vector<ft_sim3_problem> &problems, std::vector<std::vector<uint8_t>> &vbInliers) {
    std::vector<ft_sim3_result> results;
    std::vector<std::vector<uint8_t>> best;
    std::vector<std::vector<int>> counts;
    fasttrack::Sim3SolverBatch(ctx, problems, results, vbInliers, &best, &counts);
    int n = 0;
    for (size_t p = 0; p < problems.size(); p++)
        if (results[p].converged) n += results[p].n_inliers + (int)best[p].size() + (int)counts[p].size();
    return n;
}
int main() {
    ft_sim3_problem P = {};
    ft_sim3_result r = {};
    r.iterations = 7;
    uint8_t o = 7, *op = &o;
    static_assert(sizeof(r.T12) == 16 * sizeof(float) && FT_SIM3_MAX_ITERATIONS >= 2 * 300, "the reference's 300 iterations are well inside");
    return ft_sim3_solver(nullptr, 1, &P, &r, &op, nullptr, nullptr) == FT_ERR_INVALID && r.iterations == 7 && o == 7 ? 0 : 1;
}
"""


def test_cpp_mirror_of_the_sim3_solver_compiles_and_links(tmp_path):
    src = tmp_path / "sim3_solver_mirror.cpp"
    src.write_text(SRC)
    exe = tmp_path / "sim3_solver_mirror"
    lib_dir = os.path.join(ROOT, "fasttrack_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lfasttrack_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)]).returncode == 0

"""The C++ mirror of Optimizer::PoseOptimization (fasttrack::PoseOptimization, include/fasttrack_amd.hpp) compiles with plain g++
and links against the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <vector>
#include "fasttrack_amd.hpp"
// Tracking::TrackWithMotionModel for a batch of frames: the poses between the two searches, then the sweep of Tracking.cc:2992-3020
int trackBatch(fasttrack::Context &ctx, const std::vector<ft_pose_opt_frame> &frames, std::vector<std::vector<uint8_t>> &mvbOutlier,
               std::vector<ft_se3> &poses) {
    std::vector<ft_pose_opt_trace> trace;
    const std::vector<int> inliers = fasttrack::PoseOptimization(ctx, frames, poses, mvbOutlier, &trace);
    int n = 0;
    for (size_t f = 0; f < frames.size(); f++) n += inliers[f] + trace[f].iterations[0] + (int)mvbOutlier[f].size();
    return n;
}
int main() {
    ft_pose_opt_frame F = {};
    ft_se3 T = {};
    ft_pose_opt_trace tr = {};
    int n = 7;
    uint8_t o = 7, *op = &o;
    static_assert(sizeof(tr.chi2) == 4 * sizeof(double) && FT_POSE_OPT_MAX_EDGES == 2000, "four rounds");
    return ft_pose_optimization(nullptr, 1, &F, &T, &op, &n, &tr) == FT_ERR_INVALID && n == 7 && o == 7 ? 0 : 1;
}
"""


def test_cpp_mirror_of_the_pose_optimization_compiles_and_links(tmp_path):
    src = tmp_path / "pose_opt_mirror.cpp"
    src.write_text(SRC)
    exe = tmp_path / "pose_opt_mirror"
    lib_dir = os.path.join(ROOT, "fasttrack_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lfasttrack_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)]).returncode == 0

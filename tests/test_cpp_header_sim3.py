"""The C++ mirror of ORBmatcher::SearchByProjection(pKF, Scw, ...) (fasttrack::SearchByProjection, include/fasttrack_amd.hpp)
compiles with plain g++ and links against the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <vector>
#include "fasttrack_amd.hpp"
struct KeyFrame;
// LoopClosing::FindMatchesByProjection: the call with vpPointsKFs (src/LoopClosing.cc:755), then the plain one on what it left (:777)
int findMatchesByProjection(fasttrack::Context &ctx, const ft_frame_view &pCurrentKF, const fasttrack::Sim3Pose &Scw, const ft_fuse_points &vpPoints,
                            const std::vector<uint8_t> &valid, const std::vector<KeyFrame *> &vpPointsKFs, std::vector<int> &vpMatched,
                            std::vector<KeyFrame *> &vpMatchedKF) {
    int n = fasttrack::SearchByProjection(ctx, pCurrentKF, Scw, vpPoints, valid.data(), vpPointsKFs, vpMatched, vpMatchedKF, 8, 1.5f);
    std::vector<int> pointKeypoint;
    n += fasttrack::SearchByProjection(ctx, pCurrentKF, Scw, vpPoints, valid.data(), vpMatched, 5, 1.0f, &pointKeypoint);
    std::vector<ft_sim3_job> jobs(2);
    fasttrack::SearchByProjection(ctx, pCurrentKF, jobs);
    return n + jobs[0].n_matches;
}
int main() {
    ft_frame_view kf = {};
    ft_sim3_job J = {};
    int matched = 3;
    J.matched = &matched;
    J.n_matches = 7;
    static_assert(sizeof(J.Ow) == 3 * sizeof(float) && sizeof(J.th) == sizeof(int), "centre and radius");
    // a null context is an invalid argument and nothing is written
    return ft_search_keyframe_sim3(nullptr, &kf, 1, &J) == FT_ERR_INVALID && J.n_matches == 7 && matched == 3 ? 0 : 1;
}
"""


def test_cpp_mirror_of_the_sim3_search_compiles_and_links(tmp_path):
    src = tmp_path / "sim3_mirror.cpp"
    src.write_text(SRC)
    exe = tmp_path / "sim3_mirror"
    lib_dir = os.path.join(ROOT, "fasttrack_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lfasttrack_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)]).returncode == 0

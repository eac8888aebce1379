"""The C++ mirrors of ORBmatcher::SearchByProjection(Frame, KeyFrame, sAlreadyFound, th, ORBdist)
(fasttrack::TrackedFrame::SearchByProjection and fasttrack::KernelController::SearchByProjection, include/fasttrack_amd.hpp)
compile with plain g++ and link against the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <vector>
#include "fasttrack_amd.hpp"
int relocalise(fasttrack::Context &ctx, fasttrack::TrackedFrame &cur, ft_frame_view &view, const ft_keyframe_points &kf, const ft_se3 &Tcw,
               std::vector<int> &assign, std::vector<int> &bestDist) {
    // Tracking::Relocalization: th 10 / ORBdist 100, then th 3 / ORBdist 64 (src/Tracking.cc:3924, :3938)
    int n = cur.SearchByProjection(kf, Tcw, 0.1823f, 10.f, 100, true, assign);
    n += cur.SearchByProjection(kf, Tcw, 0.1823f, 3.f, 64, true, assign);
    n += fasttrack::KernelController::SearchByProjection(ctx, view, kf, Tcw, 0.1823f, 10.f, 100, true, assign);
    return n + fasttrack::KernelController::SearchByProjection(ctx, view, kf, Tcw, 0.1823f, 10.f, 100, true, assign, bestDist.data(), nullptr);
}
int main() {
    ft_keyframe_points kf = {};
    ft_se3 T = {{0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}};
    ft_frame_view F = {};
    int a = 0, n = 7;
    return ft_tracked_frame_search_keyframe_projection(nullptr, &kf, &T, 0.18f, 10.f, 100, 1, &a, &n) == FT_ERR_INVALID &&
           ft_search_keyframe_projection(nullptr, &F, &kf, &T, 0.18f, 10.f, 100, 1, &a, &n, nullptr, nullptr) == FT_ERR_INVALID && n == 7 ? 0 : 1;
}
"""


def test_cpp_mirror_of_the_relocalisation_search_compiles_and_links(tmp_path):
    src = tmp_path / "reloc_mirror.cpp"
    src.write_text(SRC)
    exe = tmp_path / "reloc_mirror"
    lib_dir = os.path.join(ROOT, "fasttrack_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lfasttrack_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)]).returncode == 0

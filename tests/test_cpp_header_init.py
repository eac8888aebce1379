"""The C++ mirror of ORBmatcher::SearchForInitialization (fasttrack::TrackedFrame::SearchForInitialization,
include/fasttrack_amd.hpp) compiles with plain g++ for a cv::Point2f-like point type and links against the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <vector>
#include "fasttrack_amd.hpp"
struct Point2f { float x, y; };
int run(fasttrack::TrackedFrame &cur, fasttrack::TrackedFrame &ini, std::vector<Point2f> &prev, std::vector<int> &m12) {
    return cur.SearchForInitialization(ini, prev, m12, 100) + cur.SearchForInitialization(ini, prev, m12, 100, 0.9f, true);
}
int main() {
    float prev[2] = {0, 0};
    int m = 0, n = 0;
    return ft_tracked_frame_search_for_initialization(nullptr, nullptr, prev, 100, 0.9f, 1, &m, &n) == FT_ERR_INVALID &&
           ft_search_for_initialization(nullptr, nullptr, nullptr, prev, 100, 0.9f, 1, &m, &n, nullptr) == FT_ERR_INVALID ? 0 : 1;
}
"""


def test_cpp_mirror_of_search_for_initialization_compiles_and_links(tmp_path):
    src = tmp_path / "init_mirror.cpp"
    src.write_text(SRC)
    exe = tmp_path / "init_mirror"
    lib_dir = os.path.join(ROOT, "fasttrack_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lfasttrack_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)]).returncode == 0

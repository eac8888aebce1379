"""The C++ mirror of ORBmatcher::SearchByBoW(KeyFrame, KeyFrame) (fasttrack::SearchByBoW over BowKeyFrame records,
include/fasttrack_amd.hpp) compiles with plain g++ and links against the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <vector>
#include "fasttrack_amd.hpp"
// LoopClosing::DetectCommonRegionsFromBoW: the current keyframe against the covisible keyframes of a candidate (src/LoopClosing.cc:657-668)
int matchCovisibles(fasttrack::Context &ctx, const fasttrack::BowKeyFrame &current, const std::vector<fasttrack::BowKeyFrame> &vpCovKFi,
                    std::vector<std::vector<int>> &vvMatches12) {
    const std::vector<int> n = fasttrack::SearchByBoW(ctx, current, vpCovKFi, 0.9f, true, vvMatches12);
    int total = 0;
    for (int v : n) total += v;
    return total;
}
// ... next to the KeyFrame, Frame overload built on the same flattening
int trackReference(fasttrack::Context &ctx, const fasttrack::ORBVocabulary::FeatureVector &a, const fasttrack::ORBVocabulary::FeatureVector &b,
                   const uint8_t *d, const std::vector<uint8_t> &has, const float *ang, std::vector<int> &m) {
    return fasttrack::SearchByBoW(ctx, a, d, 1, has, ang, b, d, 1, ang, -1, 0.7f, true, m);
}
int main() {
    static_assert(sizeof(ft_bow_keyframe) == sizeof(ft_bow_side) + sizeof(void *) + 2 * sizeof(int), "side, has_point, n_left, n_un");
    ft_bow_keyframe kf1 = {}, kf2 = {};
    kf1.n_left = kf2.n_left = -1;
    int matches12 = 3, n = 7;
    // a null context is an invalid argument and nothing is written
    return ft_search_by_bow_keyframes(nullptr, &kf1, 1, &kf2, 0.9f, 1, &matches12, &n) == FT_ERR_INVALID && matches12 == 3 && n == 7 ? 0 : 1;
}
"""


def test_cpp_mirror_of_the_keyframe_bow_search_compiles_and_links(tmp_path):
    src = tmp_path / "bow_kf_mirror.cpp"
    src.write_text(SRC)
    exe = tmp_path / "bow_kf_mirror"
    lib_dir = os.path.join(ROOT, "fasttrack_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lfasttrack_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)]).returncode == 0

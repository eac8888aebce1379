"""The C++ mirror of the relocalisation loop over ORBmatcher::SearchByBoW(KeyFrame, Frame) (fasttrack::SearchByBoW over
BowCandidate records, include/fasttrack_amd.hpp) compiles with plain g++ and links against the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <vector>
#include "fasttrack_amd.hpp"
// Tracking::Relocalization: the current frame against every candidate keyframe (src/Tracking.cc:3839-3860)
int matchCandidates(fasttrack::Context &ctx, const std::vector<fasttrack::BowCandidate> &vpCandidateKFs,
                    const fasttrack::ORBVocabulary::FeatureVector &frameFeatVec, const uint8_t *frameDescriptors, int N, const float *angles,
                    std::vector<std::vector<int>> &vvMatches) {
    const std::vector<int> n = fasttrack::SearchByBoW(ctx, vpCandidateKFs, frameFeatVec, frameDescriptors, N, angles, -1, false, 0.75f, true, vvMatches);
    int kept = 0;
    for (int v : n) kept += v >= 15;
    return kept;
}
int main() {
    static_assert(sizeof(ft_bow_candidate) == sizeof(ft_bow_side) + sizeof(void *), "side, has_point");
    ft_bow_side frame = {};
    ft_bow_candidate kf = {};
    int matches = 3, n = 7;
    // a null context is an invalid argument and nothing is written
    return ft_search_by_bow_candidates(nullptr, &frame, -1, 0, 1, &kf, 0.75f, 1, &matches, &n) == FT_ERR_INVALID && matches == 3 && n == 7 ? 0 : 1;
}
"""


def test_cpp_mirror_of_the_relocalisation_bow_search_compiles_and_links(tmp_path):
    src = tmp_path / "bow_reloc_mirror.cpp"
    src.write_text(SRC)
    exe = tmp_path / "bow_reloc_mirror"
    lib_dir = os.path.join(ROOT, "fasttrack_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lfasttrack_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)]).returncode == 0

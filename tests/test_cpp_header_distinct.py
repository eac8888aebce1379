"""The C++ mirror of MapPoint::ComputeDistinctiveDescriptors (fasttrack::ComputeDistinctiveDescriptors over per-point lists of
descriptor rows, include/fasttrack_amd.hpp) compiles with plain g++ and links against the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <vector>
#include "fasttrack_amd.hpp"
// LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:312-323): one call for the map points of the new keyframe
int updateDescriptors(fasttrack::Context &ctx, const std::vector<std::vector<const uint8_t *>> &vvDescriptors,
                      std::vector<fasttrack::Descriptor256> &mDescriptors) {
    std::vector<int> medians;
    const std::vector<int> best = fasttrack::ComputeDistinctiveDescriptors(ctx, vvDescriptors, mDescriptors, &medians);
    int n = 0;
    for (size_t p = 0; p < best.size(); p++) n += best[p] >= 0 && medians[p] >= 0;
    return n + (int)fasttrack::ComputeDistinctiveDescriptors(ctx, vvDescriptors, mDescriptors).size();
}
int main() {
    static_assert(FT_DISTINCT_MAX_OBSERVATIONS >= 1024, "the per-point cap");
    static_assert(sizeof(fasttrack::Descriptor256) == 32, "a descriptor row");
    const int offsets[2] = {0, 1};
    const uint8_t d[32] = {};
    int best = 3, median = 7;
    uint8_t out[32];
    for (int i = 0; i < 32; i++) out[i] = 0xAB;
    // a null context is an invalid argument and nothing is written
    if (ft_distinctive_descriptors(nullptr, 1, offsets, d, &best, &median, out) != FT_ERR_INVALID) return 1;
    for (int i = 0; i < 32; i++)
        if (out[i] != 0xAB) return 2;
    return best == 3 && median == 7 ? 0 : 3;
}
"""


def test_cpp_mirror_of_the_distinctive_descriptors_compiles_and_links(tmp_path):
    src = tmp_path / "distinct_mirror.cpp"
    src.write_text(SRC)
    exe = tmp_path / "distinct_mirror"
    lib_dir = os.path.join(ROOT, "fasttrack_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lfasttrack_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)]).returncode == 0

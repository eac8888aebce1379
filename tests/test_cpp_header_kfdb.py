"""The C++ mirror of KeyFrameDatabase (fasttrack::KeyFrameDatabase with the reference's names - add, erase, clear,
DetectNBestCandidates, DetectRelocalizationCandidates - include/fasttrack_amd.hpp) compiles with plain g++ and links against the
library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <map>
#include <vector>
#include "fasttrack_amd.hpp"
struct KF { int handle, map; long long mnId; fasttrack::ORBVocabulary::BowVector mBowVec; std::vector<int> covisible, connected; };
// LoopClosing::NewDetectCommonRegions (src/LoopClosing.cc:491): the place-recognition query of the current keyframe
int detect(fasttrack::KeyFrameDatabase &db, std::map<int, KF> &kfs, KF &cur, std::vector<int> &vpLoopBowCand, std::vector<int> &vpMergeBowCand) {
    db.DetectNBestCandidates(cur.mnId, cur.mBowVec, cur.connected, cur.map, [&](int h) { return kfs[h].covisible; },
                             [&](int h) { return kfs[h].map; }, vpLoopBowCand, vpMergeBowCand, 3);
    cur.handle = db.add(cur.mBowVec);   // LoopClosing.cc:522
    return (int)(vpLoopBowCand.size() + vpMergeBowCand.size());
}
// Tracking::Relocalization (src/Tracking.cc:3810)
std::vector<int> relocalize(fasttrack::KeyFrameDatabase &db, std::map<int, KF> &kfs, long long frameId,
                            const fasttrack::ORBVocabulary::BowVector &bow, int currentMap) {
    return db.DetectRelocalizationCandidates(frameId, bow, currentMap, [&](int h) { return kfs[h].covisible; }, [&](int h) { return kfs[h].map; });
}
void forget(fasttrack::KeyFrameDatabase &db, const KF &kf, const std::vector<int> &mapHandles) {
    db.erase(kf.handle);     // KeyFrame::SetBadFlag
    db.erase(mapHandles);    // clearMap
    db.clear();
    (void)db.size();
}
int main() {
    static_assert(FT_KFDB_MAX_QUERY_WORDS >= 4000, "2 x nFeatures words fit a query");
    ft_kfdb *db = reinterpret_cast<ft_kfdb *>(&db);
    // a null context and an unknown scoring are invalid arguments, and nothing is written
    if (ft_kfdb_create(nullptr, 0, &db) != FT_ERR_INVALID || db != reinterpret_cast<ft_kfdb *>(&db)) return 1;
    int n = 7, h = 9;
    long long w = 11;
    if (ft_kfdb_size(nullptr, &n, &w) != FT_ERR_INVALID || n != 7 || w != 11) return 2;
    if (ft_kfdb_erase(nullptr, 1, &h) != FT_ERR_INVALID || ft_kfdb_clear(nullptr) != FT_ERR_INVALID) return 3;
    int ns = 1, mx = 2, mn = 3, nsc = 4;
    if (ft_kfdb_score(nullptr, 0, 1, 0, nullptr, nullptr, 0, nullptr, &ns, &mx, &mn, &nsc, nullptr, nullptr, nullptr, nullptr) != FT_ERR_INVALID)
        return 4;
    if (ft_kfdb_select_reloc(nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &n) != FT_ERR_INVALID) return 5;
    if (ft_kfdb_select_n_best(nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 3, nullptr, &n, nullptr, &h) !=
        FT_ERR_INVALID)
        return 6;
    return ns == 1 && mx == 2 && mn == 3 && nsc == 4 && n == 7 && h == 9 && ft_kfdb_destroy(nullptr) == FT_OK ? 0 : 7;
}
"""


def test_cpp_mirror_of_the_keyframe_database_compiles_and_links(tmp_path):
    src = tmp_path / "kfdb_mirror.cpp"
    src.write_text(SRC)
    exe = tmp_path / "kfdb_mirror"
    lib_dir = os.path.join(ROOT, "fasttrack_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lfasttrack_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)]).returncode == 0

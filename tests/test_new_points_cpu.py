"""Pins tests/new_points_ref.py, the restatement of the triangulation loop of LocalMapping::CreateNewMapPoints that the GPU tests
compare the device with, and asserts that the shared cases exercise what they claim - so that the GPU tests cannot pass vacuously."""
import functools

import numpy as np

from tests import new_points_cases as nc
from tests import new_points_ref as npr

f32 = np.float32


@functools.lru_cache(maxsize=None)
def reference(key):
    S = nc.scenario(*key)
    return npr.triangulate_new_points(S["kf1"], S["g1"], S["neighbours"], S["geometries"], S["matches12"], **S["params"])


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_null_vector_and_accepted_points_against_numpy_svd_and_the_truth():
    """exact projections of known points: the restated null vector gives the x3D of np.linalg.svd (float64) on the same matrix A, and
    an accepted x3D is the ground truth; tolerances: new_points_cases.NULLVEC_TOL / TRUTH_TOL (measured, times 4)"""
    worst_svd = worst_truth = worst_svd_truth = 0.0
    checked = 0
    for S in nc.exact_cases():
        r = npr.triangulate_new_points(S["kf1"], S["g1"], S["neighbours"], S["geometries"], S["matches12"], **S["params"])
        for k, (kf2, g2) in enumerate(zip(S["neighbours"], S["geometries"])):
            for idx1 in np.nonzero(r["status"][k] > 0)[0]:
                truth = S["truth"][idx1]
                worst_truth = max(worst_truth, _rel(r["x3d"][k, idx1], truth))
                if r["status"][k, idx1] != 1:
                    continue
                info = {}
                idx2 = int(S["matches12"][k, idx1])
                npr.new_point(S["kf1"], S["g1"], kf2, g2, int(idx1), idx2, False, False, 0.0, nc.RATIO_FACTOR, info)
                A = np.array([float(v) for v in info["A"]]).reshape(4, 4)
                v = np.linalg.svd(A)[2][3]
                ours = np.array(npr.null_vector4(info["A"]))
                worst_svd = max(worst_svd, _rel(ours[:3] / ours[3], v[:3] / v[3]))
                worst_svd_truth = max(worst_svd_truth, _rel(v[:3] / v[3], truth))
                checked += 1
    print(f"null vector vs numpy svd {worst_svd:.3g}, numpy svd vs truth {worst_svd_truth:.3g}, accepted x3D vs truth {worst_truth:.3g} "
          f"over {checked} triangulated points")
    assert checked >= 200
    assert worst_svd <= nc.NULLVEC_TOL
    assert worst_truth <= nc.TRUTH_TOL


def test_exact_cases_accept_every_pair_with_parallax():
    """true correspondences without noise: accepted, or (the pinhole form's near neighbour, features without mvuRight) low parallax"""
    for S in nc.exact_cases():
        r = npr.triangulate_new_points(S["kf1"], S["g1"], S["neighbours"], S["geometries"], S["matches12"], **S["params"])
        assert set(np.unique(r["status"]).tolist()) <= {1, 2, 3, -1}, np.unique(r["status"])
        assert (r["status"][0] > 0).all()
        assert (r["first_neighbour"] == 0).all()


def test_directed_cases_have_the_status_the_reference_text_gives():
    seen = set()
    for c in nc.directed():
        r = npr.triangulate_new_points(c["kf1"], c["g1"], [c["kf2"]], [c["g2"]], c["matches12"], **c["params"])
        assert np.array_equal(r["status"][0], c["status"]), (c["name"], r["status"][0])
        assert np.array_equal(r["x3d"][0][c["status"] <= 0], np.zeros((int((c["status"] <= 0).sum()), 3), f32)), c["name"]
        seen |= set(c["status"].tolist())
    assert seen | {0} == set(nc.REACHABLE)


def test_the_four_pairings_take_the_four_poses():
    c = nc.four_pairings()
    for i in range(4):
        info = {}
        st, x = npr.new_point(c["kf1"], c["g1"], c["kf2"], c["g2"], i, int(c["matches12"][0, i]), False, False, 0.0, nc.RATIO_FACTOR, info)
        assert st == 1 and info["pairing"] == c["pairings"][i]
        assert _rel(x, c["truth"][i]) <= nc.TRUTH_TOL


def test_stereo_parallax_is_an_else_if():
    c = next(c for c in nc.hand_built() if c["name"] == "both_stereo_else_if")
    info = {}
    npr.new_point(c["kf1"], c["g1"], c["kf2"], c["g2"], 0, 0, False, False, 0.0, nc.RATIO_FACTOR, info)
    assert info["stereo"] == (True, True)
    cs1, cs2 = info["cos_stereo"]
    assert cs2 == f32(info["cos_rays"] + f32(1)) and cs1 < 1  # keyframe 2's cosine was never computed


def test_scenarios_reach_every_status_and_every_neighbour_accepts():
    seen = set()
    for key in nc.MAIN:
        r = reference(key)
        for k in range(key[3]):
            assert (r["status"][k] == 1).any(), (key, k)
        seen |= set(np.unique(r["status"]).tolist())
        if key[0] == "pinhole" and key[3] > 1:
            assert (r["status"] == 2).any() and (r["status"] == 3).any(), key
        assert np.array_equal(r["n_points"], (r["status"] > 0).sum(1))
        assert (r["first_neighbour"] >= 1).any() or key[3] == 1, key  # a later neighbour wins for some feature
        taken = (r["status"] > 0).sum(0)
        assert (taken >= 2).any() or key[3] == 1, key                   # ... and some feature is accepted by several
    for c in nc.directed():
        seen |= set(c["status"].tolist())
    assert seen == set(nc.REACHABLE), sorted(set(nc.REACHABLE) - seen)


def test_batched_rows_equal_the_single_neighbour_calls():
    for key in nc.MAIN[:3]:
        S, r = nc.scenario(*key), reference(key)
        first = np.full(len(S["kf1"]["keys"]), -1, np.int32)
        for k in range(key[3]):
            r1 = npr.triangulate_new_points(S["kf1"], S["g1"], [S["neighbours"][k]], [S["geometries"][k]], S["matches12"][k:k + 1], **S["params"])
            assert np.array_equal(r1["status"][0], r["status"][k]) and np.array_equal(r1["x3d"][0], r["x3d"][k])
            assert r1["n_points"][0] == r["n_points"][k]
            first = np.where((first < 0) & (r1["first_neighbour"] == 0), k, first)
        assert np.array_equal(first, r["first_neighbour"])


def test_boundary_rows_hold_their_counts_in_the_chunks_they_claim():
    S, rows = nc.boundary_rows("pinhole")
    assert len(S["kf1"]["keys"]) == 600 and (S["matches12"][0] >= 0).all()
    per_chunk = {c: [int((row[o:o + nc.CHUNK] >= 0).sum()) for o in range(0, 600, nc.CHUNK)] for c, row in rows.items()}
    assert per_chunk == {0: [0, 0, 0], 1: [0, 0, 1], 63: [32, 31, 0], 64: [32, 32, 0], 65: [32, 33, 0], 257: [1, 256, 0]}

"""The restatement of ORBmatcher::Fuse (tests/fuse_ref.py) and the inputs of its tests (tests/fuse_cases.py), without a GPU:
the restatement's geometry against the oracle's isInFrustum, the hand-built cases against expectations written out from the
reference text, the conditions the random cases must meet, and the caller's apply loop against the reference's inline bookkeeping."""
import numpy as np
import pytest

from oracle import binding as ob
from tests import fuse_cases as fc
from tests import fuse_ref as ref

P320 = fc.RANDOM[0]


def test_geometry_agrees_with_is_in_frustum():
    """Projection, distance range, PO.dot(Pn) and level against Frame::isInFrustum (left camera, viewing_cos_limit 0.5) where the two
    functions test the same thing: isInFrustum wants z > 0 and `<`/`>` bounds, divides the dot by the distance before it compares
    - points it accepts must be accepted here with the same projection and level; points this one searches and it rejects must
    sit on one of those differences."""
    for name in (P320, "kb8mono"):
        case = fc.random_case(name)
        oF, _ = case["view"](device=False)
        r = fc.expected(case, 3.0, True)
        T = case["Tcw"].matrix()
        pose = ob.make_pose(T[:, :3], T[:, 3])
        pose.Ow[:] = [float(v) for v in case["Ow"]]
        fr = ob.is_in_frustum(oF, pose, case["points"], 0.5, case["log_sf"])
        reached = (r["stage"] == ref.SEARCHED) | (r["stage"] == ref.EMPTY)
        # the oracle transforms with the rotation matrix, the restatement in the Sophus form: projections agree to float noise
        both = reached & (fr["in_view"] != 0)
        assert both.sum() >= 200
        assert np.allclose(r["u"][both], fr["proj_x"][both], atol=2e-3) and np.allclose(r["v"][both], fr["proj_y"][both], atol=2e-3)
        assert np.array_equal(r["level"][both], fr["level"][both])
        assert np.allclose(r["dot"][both] / r["dist"][both], fr["view_cos"][both], atol=1e-6)
        valid = case["valid"] != 0
        only_frustum = valid & (fr["in_view"] != 0) & ~reached
        only_fuse = valid & reached & (fr["in_view"] == 0)
        print(name, "both", int(both.sum()), "only isInFrustum", int(only_frustum.sum()), "only Fuse", int(only_fuse.sum()))
        for i in np.nonzero(only_frustum | only_fuse)[0]:   # a rounding border of one of the tests, never a different decision
            border = min(abs(r["u"][i] - oF.c.mnMinX), abs(r["u"][i] - oF.c.mnMaxX), abs(r["v"][i] - oF.c.mnMinY), abs(r["v"][i] - oF.c.mnMaxY)) < 1e-2
            cos_border = np.isfinite(r["dot"][i]) and abs(r["dot"][i] / r["dist"][i] - 0.5) < 1e-6
            assert border or cos_border or abs(r["zc"][i]) < 1e-6, (name, i)


@pytest.mark.parametrize("name", sorted(fc.hand_cases()))
def test_hand_case(name):
    case = fc.hand_cases()[name]
    r = fc.run_hand_case(case)
    for k in ("best_idx", "best_dist", "stage"):
        assert r[k].tolist() == case["expect"][k], (name, k, r[k].tolist())
    assert r["n_found"] == case["expect"]["n_found"]


@pytest.mark.parametrize("name", fc.RANDOM)
def test_random_cases_meet_their_conditions(name):
    """conditions on the inputs (th 3, SE3 overload), not measurements: every exit is taken, matches are found, the chi-square test
    rejects and changes outcomes"""
    case = fc.random_case(name)
    r = fc.expected(case, 3.0, True)
    st = r["stats"]
    print(name, st, "n_found", r["n_found"])
    for s in range(1, 6):
        assert st["stages"][s] >= 10, (name, s, st["stages"])
    if name == P320:
        assert st["stages"][ref.EMPTY] >= 10
    assert r["n_found"] >= 50
    assert st["chi_stereo"] + st["chi_mono"] >= 100
    assert st["changed_by_chi"] >= 30
    if name == P320:
        assert st["chi_stereo"] > 0 and st["chi_mono"] > 0   # the rectified frame has both kinds of keypoints
    s4 = fc.expected(case, 4.0, False)
    assert s4["stats"]["chi_stereo"] + s4["stats"]["chi_mono"] == 0 and s4["n_found"] >= 50


def test_cell_crowd_windows():
    for n in (1, 15, 16, 17, 63, 64, 65, 130):
        c = fc.cell_crowd(n)
        r = fc.run_hand_case(c)
        assert r["stats"]["max_window"] == n + 3 and r["stage"][0] == 0
        assert r["best_dist"][0] == 1 and r["best_idx"][0] == max(n // 2 - 1, 0)


def test_apply_loop_equals_inline_bookkeeping():
    """A one-target search of the list as it stands at call time followed by the in-order apply loop (which re-tests isBad /
    IsInKeyFrame) is Fuse with its bookkeeping inline: a list with duplicates, points already in the keyframe and bad points."""
    case = fc.random_case(P320)
    oF, _ = case["view"](device=False)
    pts, M = case["points"], len(case["valid"])
    rng = np.random.default_rng(5)
    base = fc.expected(case, 3.0, True)
    good = np.nonzero(base["best_dist"] <= ref.TH_LOW)[0]
    assert len(good) >= 50
    # the list: every point, then 60 of the matching ones a second time (the same MapPoint listed twice)
    again = rng.choice(good, 60, replace=False)
    order = np.concatenate([np.arange(M), again])
    listed = {k: np.asarray(v)[order] for k, v in pts.items()}

    def world():
        objs = [ref.MP(i, int(rng2.integers(0, 5))) for i in range(M)]
        for i in range(M):
            if not case["valid"][i]:
                objs[i].bad = True
        slots = {}
        for kp in rng2.choice(oF.N, oF.N // 3, replace=False):   # a third of the keypoints hold a point of their own
            slots[int(kp)] = ref.MP(-1 - int(kp), int(rng2.integers(0, 5)))
        for i in rng2.choice(good, 10, replace=False):          # ten listed points are in the keyframe already
            objs[i].in_kf = True
        return [objs[i] for i in order], slots

    rng2 = np.random.default_rng(6)
    vp_a, slots_a = world()
    rng2 = np.random.default_rng(6)
    vp_b, slots_b = world()
    n_inline = ref.fuse_inline(oF, listed, vp_a, slots_a, case["Tcw"], case["Ow"], case["log_sf"], 3.0)
    valid = np.array([0 if (p.bad or p.in_kf) else 1 for p in vp_b], np.uint8)
    res = ref.fuse(oF, listed, case["Tcw"], case["Ow"], case["log_sf"], 3.0, valid=valid)
    n_apply = ref.apply_in_order(res, vp_b, slots_b)
    assert n_inline == n_apply and n_inline >= 40
    state = lambda vp, slots: ([(p.bad, p.in_kf, p.obs, None if p.replaced is None else p.replaced.i) for p in vp],
                               sorted((k, v.i) for k, v in slots.items()))
    assert state(vp_a, slots_a) == state(vp_b, slots_b)
    # and the re-test matters: applying without it fuses the second listing of a point again
    skipped_at_apply = sum(1 for i, p in enumerate(vp_b) if valid[i] and res["best_dist"][i] <= ref.TH_LOW and i >= M)
    assert skipped_at_apply >= 10 and n_apply < int((res["best_dist"] <= ref.TH_LOW).sum())

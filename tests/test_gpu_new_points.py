"""ft_triangulate_new_points / ft_search_and_triangulate on the device against the restatement of the triangulation loop of
LocalMapping::CreateNewMapPoints (tests/new_points_ref.py): status, x3d, n_points and first_neighbour bit for bit, no tolerance and
no excluded case (the device runs the null_vector4 the restatement states; test_new_points_cpu.py pins the restatement)."""
import functools

import numpy as np
import pytest

from fasttrack_amd import orb
from tests import new_points_cases as nc
from tests import new_points_ref as npr
from tests import triangulation_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def run(ctx, kf1, g1, kfs, gs, m12, params):
    return orb.triangulate_new_points(ctx, tc.to_device(orb, kf1), nc.to_device_geometry(orb, g1), [tc.to_device(orb, k) for k in kfs],
                                      [nc.to_device_geometry(orb, g) for g in gs], m12, params["inertial"], params["far_points"],
                                      params["th_far"], params["ratio_factor"])


@functools.lru_cache(maxsize=None)
def reference(key):
    S = nc.scenario(*key)
    return npr.triangulate_new_points(S["kf1"], S["g1"], S["neighbours"], S["geometries"], S["matches12"], **S["params"])


def check(tag, got, want):
    assert np.array_equal(got["status"], want["status"]), (tag, np.argwhere(got["status"] != want["status"])[:10])
    assert np.array_equal(got["x3d"].view(np.uint32), want["x3d"].view(np.uint32)), (tag, np.argwhere(got["x3d"] != want["x3d"])[:10])
    assert np.array_equal(got["n_points"], want["n_points"]), (tag, got["n_points"], want["n_points"])
    assert np.array_equal(got["first_neighbour"], want["first_neighbour"]), tag


@pytest.mark.parametrize("form,seed,n1,nn", nc.MAIN)
def test_scenarios_match_the_restatement(ctx, form, seed, n1, nn):
    S = nc.scenario(form, seed, n1, nn)
    want = reference((form, seed, n1, nn))
    check((form, seed), run(ctx, S["kf1"], S["g1"], S["neighbours"], S["geometries"], S["matches12"], S["params"]), want)
    for inertial, far in ((True, False), (True, True)):
        P = dict(S["params"], inertial=inertial, far_points=far, th_far=3.0)
        check((form, seed, inertial, far), run(ctx, S["kf1"], S["g1"], S["neighbours"], S["geometries"], S["matches12"], P),
              npr.triangulate_new_points(S["kf1"], S["g1"], S["neighbours"], S["geometries"], S["matches12"], **P))


def test_batched_call_equals_the_single_neighbour_calls(ctx):
    key = nc.MAIN[2]
    S, want = nc.scenario(*key), reference(key)
    for k in range(key[3]):
        g = run(ctx, S["kf1"], S["g1"], [S["neighbours"][k]], [S["geometries"][k]], S["matches12"][k:k + 1], S["params"])
        assert np.array_equal(g["status"][0], want["status"][k]) and np.array_equal(g["x3d"][0], want["x3d"][k])
        assert g["n_points"][0] == want["n_points"][k]
        assert np.array_equal(g["first_neighbour"], np.where(want["status"][k] > 0, 0, -1))


@pytest.mark.parametrize("case", nc.directed(), ids=lambda c: c["name"])
def test_directed_cases(ctx, case):
    want = npr.triangulate_new_points(case["kf1"], case["g1"], [case["kf2"]], [case["g2"]], case["matches12"], **case["params"])
    assert np.array_equal(want["status"][0], case["status"])
    g = run(ctx, case["kf1"], case["g1"], [case["kf2"]], [case["g2"]], case["matches12"], case["params"])
    assert np.array_equal(g["status"][0], case["status"]), g["status"][0]
    check(case["name"], g, want)


@pytest.mark.parametrize("form", nc.FORMS)
def test_match_counts_at_wave_and_workgroup_boundaries(ctx, form):
    """0, 1, 63, 64, 65 and 257 matches in a row of 600, in different chunks and across their borders; the counts as separate
    calls and as the six neighbours of one"""
    S, rows = nc.boundary_rows(form)
    full = reference((form, 60, 600, 1, True))
    kf2, g2 = S["neighbours"][0], S["geometries"][0]

    def cut(row):
        keep = row >= 0
        st = np.where(keep, full["status"][0], 0).astype(np.int32)
        return st, np.where(keep[:, None] & (st > 0)[:, None], full["x3d"][0], np.float32(0)).astype(np.float32)

    sts, xs = zip(*[cut(rows[c]) for c in nc.COUNTS])
    for c, st, x in zip(nc.COUNTS, sts, xs):
        assert int((st != 0).sum()) == c
        want = dict(status=st[None], x3d=x[None], n_points=np.array([(st > 0).sum()], np.int32), first_neighbour=np.where(st > 0, 0, -1).astype(np.int32))
        check((form, c), run(ctx, S["kf1"], S["g1"], [kf2], [g2], rows[c][None], S["params"]), want)
    st, nb = np.stack(sts), len(nc.COUNTS)
    acc = st > 0
    want = dict(status=st, x3d=np.stack(xs), n_points=acc.sum(1).astype(np.int32),
                first_neighbour=np.where(acc.any(0), acc.argmax(0), -1).astype(np.int32))
    check((form, "all"), run(ctx, S["kf1"], S["g1"], [kf2] * nb, [g2] * nb, np.stack([rows[c] for c in nc.COUNTS]), S["params"]), want)


def test_unread_fields_may_be_null(ctx):
    """the stand-alone stage reads neither descriptors nor the FeatureVector nor has_point"""
    key = nc.MAIN[0]
    S = nc.scenario(*key)
    k1, k2 = tc.to_device(orb, S["kf1"]), [tc.to_device(orb, k) for k in S["neighbours"]]
    for k in [k1] + k2:
        k.c.descriptors = k.c.has_point = k.c.fv_nodes = k.c.fv_offsets = k.c.fv_features = None
        k.c.n_nodes = 0
    P = S["params"]
    g = orb.triangulate_new_points(ctx, k1, nc.to_device_geometry(orb, S["g1"]), k2, [nc.to_device_geometry(orb, g) for g in S["geometries"]],
                                   S["matches12"], P["inertial"], P["far_points"], P["th_far"], P["ratio_factor"])
    check("null fields", g, reference(key))


def _search_inputs(form, seed, neighbours=None):
    S = tc.scenario(form, seed)
    ks = list(range(len(S["neighbours"]))) if neighbours is None else neighbours
    kf1, kfs, pairs = S["kf1"], [S["neighbours"][k] for k in ks], [S["pairs"][k] for k in ks]
    g1 = nc.geometry_from_pair(kf1, pairs[0], True)
    gs = [nc.geometry_from_pair(k, p, False) for k, p in zip(kfs, pairs)]
    return (tc.to_device(orb, kf1), nc.to_device_geometry(orb, g1), [tc.to_device(orb, k) for k in kfs], [nc.to_device_geometry(orb, g) for g in gs],
            [tc.to_device_pair(orb, p) for p in pairs])


@pytest.mark.parametrize("form,seed", [("pinhole", 11), ("kb8", 13), ("kb8x2", 14)])
def test_fused_call_equals_the_two_calls(ctx, form, seed):
    """ft_search_and_triangulate = ft_search_for_triangulation, then ft_triangulate_new_points on its rows: every output"""
    k1, g1, k2, g2, pairs = _search_inputs(form, seed)
    for flags in ((False, False, True), (False, True, False)):
        s = orb.search_for_triangulation(ctx, k1, k2, pairs, *flags)
        t = orb.triangulate_new_points(ctx, k1, g1, k2, g2, s["matches12"], False, True, 40.0, nc.RATIO_FACTOR)
        f = orb.search_and_triangulate(ctx, k1, g1, k2, g2, pairs, *flags, inertial=False, far_points=True, th_far_points=40.0,
                                       ratio_factor=nc.RATIO_FACTOR)
        for name in ("matches12", "n", "best_dist"):
            assert np.array_equal(f[name], s[name]), (form, flags, name)
        check((form, flags), f, t)
        assert (t["n_points"] > 0).all() and (s["n"] >= 100).all(), (t["n_points"], s["n"])


def test_launch_counts_are_fixed(ctx):
    """3 kernels per fused call for one neighbour and for three, 1 per stand-alone call; the matcher keeps its 2"""
    try:
        ctx.set_kernel_timing(True)
        ctx.reset_stats()
        for nbrs, calls in (([0], 1), ([0, 1, 2], 2)):
            k1, g1, k2, g2, pairs = _search_inputs("pinhole", 11, nbrs)
            f = orb.search_and_triangulate(ctx, k1, g1, k2, g2, pairs, ratio_factor=nc.RATIO_FACTOR)
            assert ctx.get_stat("search_and_triangulate.launches") == (3.0 * calls, calls)
            orb.triangulate_new_points(ctx, k1, g1, k2, g2, f["matches12"], ratio_factor=nc.RATIO_FACTOR)
            assert ctx.get_stat("triangulate_new_points.launches") == (1.0 * calls, calls)
        assert ctx.get_stat("kernel.triang_points")[1] == 4
        for name in ("kernel.triang_match", "kernel.triang_finish"):
            assert ctx.get_stat(name)[1] == 2, name
        orb.search_for_triangulation(ctx, k1, k2, pairs)
        assert ctx.get_stat("search_for_triangulation.launches") == (2.0, 1)
        assert ctx.get_stat("kernel.triang_points")[1] == 4
    finally:
        ctx.set_kernel_timing(False)


def test_empty_inputs_return_without_a_launch(ctx):
    S = nc.scenario(*nc.MAIN[0])
    empty = nc._keyframe(tc._keys([], [], []), 0, tc.PINHOLE_CAM)
    ge = nc.geometry(np.eye(4), tc.PINHOLE_CAM)
    ctx.reset_stats()
    g = run(ctx, empty, ge, S["neighbours"], S["geometries"], np.zeros((3, 0), np.int32), S["params"])
    assert g["n_points"].tolist() == [0, 0, 0] and g["status"].shape == (3, 0) and g["first_neighbour"].shape == (0,)
    g = run(ctx, S["kf1"], S["g1"], [], [], np.zeros((0, len(S["kf1"]["keys"])), np.int32), S["params"])
    assert len(g["n_points"]) == 0 and (g["first_neighbour"] == -1).all()
    k1, g1, k2, g2, pairs = _search_inputs("pinhole", 11)
    f = orb.search_and_triangulate(ctx, k1, g1, [], [], [])
    assert len(f["n"]) == 0 and len(f["n_points"]) == 0
    assert ctx.get_stat("triangulate_new_points.launches") == (0.0, 0) and ctx.get_stat("search_and_triangulate.launches") == (0.0, 0)
    # a neighbour without features and a row without matches still take the launch, and give zeros
    g = run(ctx, S["kf1"], S["g1"], [empty], [ge], np.full((1, len(S["kf1"]["keys"])), -1, np.int32), S["params"])
    assert not g["status"].any() and not g["x3d"].any() and g["n_points"].tolist() == [0] and (g["first_neighbour"] == -1).all()


def test_bad_arguments_raise(ctx):
    key = nc.MAIN[0]
    S = nc.scenario(*key)
    kf1, kf2, g1, g2, m = S["kf1"], S["neighbours"][0], S["g1"], S["geometries"][0], S["matches12"][:1]

    def bad(m12=m, g1_=g1, g2_=g2, which=2, **kw):
        a, b = (dict(kf1, **kw), kf2) if which == 1 else (kf1, dict(kf2, **kw))
        with pytest.raises(orb.FastTrackError) as e:
            run(ctx, a, g1_, [b], [g2_], m12, S["params"])
        assert e.value.status == -1, kw
    m2 = m.copy()
    m2[0, np.nonzero(m2[0] >= 0)[0][0]] = len(kf2["keys"])
    bad(m12=m2)                                                  # a matches12 entry >= kf2.n
    bad(g2_=dict(g2, depth=None))                                # uright >= 0 without depth
    bad(g1_=dict(g1, depth=None))
    bad(two_cameras=True)                                        # a pinhole keyframe with two cameras
    bad(cam_model=1)                                             # the keyframes of a call differ in the camera model
    k = kf2["keys"].copy()
    k["octave"][5] = tc.NLEVELS
    bad(keys=k)                                                  # an octave outside [0, nlevels)
    k = kf1["keys"].copy()
    k["octave"][0] = -1
    bad(keys=k, which=1)
    bad(n_left=len(kf2["keys"]) + 1)                             # n_left out of range
    S2 = nc.scenario(*nc.MAIN[2])                                # two_cameras on one side only
    with pytest.raises(orb.FastTrackError):
        run(ctx, S2["kf1"], S2["g1"], [dict(S2["neighbours"][0], two_cameras=False)], [S2["geometries"][0]], S2["matches12"][:1], S2["params"])
    check("after the errors", run(ctx, S["kf1"], S["g1"], S["neighbours"], S["geometries"], S["matches12"], S["params"]), reference(key))

"""ft_pose_optimization on the device against the restatement of Optimizer::PoseOptimization (tests/pose_opt_ref.py): mvbOutlier,
the return value and the integers of the trace equal, the pose within POSE_TOL, currentChi within the same relative tolerance - and,
because the kernel sums in the restatement's order and evaluates the same written-out sin / cos / atan2, every bit of both equal;
independence from the batch, repeatability, pinned inputs, invalid arguments."""
import ctypes as C

import numpy as np
import pytest

from fasttrack_amd import _capi, orb
from tests import pose_opt_cases as pc
from tests import pose_opt_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def run(ctx, keys, pinned=None, outlier=None):
    return orb.pose_optimization(ctx, [pc.to_device(orb, pc.ALL[k], outlier=outlier, pinned=pinned) for k in keys])


def normalised(q):
    """the reference's own sign normalisation (SE3Quat::normalizeRotation): w >= 0"""
    return -q if q[3] < 0 else q


def check(key, got, want):
    assert np.array_equal(got["outlier"], want["outlier"]), (key, np.nonzero(got["outlier"] != want["outlier"])[0][:10])
    assert got["ret"] == want["ret"], (key, got["ret"], want["ret"])
    assert [t[:2] for t in got["trace"]] == [t[:2] for t in want["trace"]], (key, got["trace"], want["trace"])
    assert pc.pose_close(normalised(got["Tcw"][0]), normalised(want["Tcw"][0])) and pc.pose_close(got["Tcw"][1], want["Tcw"][1]), (key, got["Tcw"], want["Tcw"])
    for g, w in zip(got["trace"], want["trace"]):
        assert abs(g[2] - w[2]) <= pc.CHI_RTOL * abs(w[2]), (key, g, w)


def same_bits(a, b):
    return (np.array_equal(a["Tcw"][0].view(np.uint32), b["Tcw"][0].view(np.uint32)) and np.array_equal(a["Tcw"][1].view(np.uint32), b["Tcw"][1].view(np.uint32))
            and np.array_equal(a["outlier"], b["outlier"]) and a["ret"] == b["ret"] and
            [(t[0], t[1], np.float64(t[2]).view(np.uint64)) for t in a["trace"]] == [(t[0], t[1], np.float64(t[2]).view(np.uint64)) for t in b["trace"]])


@pytest.fixture(scope="module")
def all_cases(ctx):
    """every committed case and every tracking frame in one call (a batch of 23 frames of every size and model)"""
    return dict(zip(pc.ALL, run(ctx, list(pc.ALL))))


@pytest.mark.parametrize("key", list(pc.ALL))
def test_case_matches_the_restatement(all_cases, key):
    check(key, all_cases[key], pc.reference(key))


@pytest.mark.parametrize("key", list(pc.ALL))
def test_case_is_the_restatement_bit_for_bit(all_cases, key):
    """the sums in g2o's order, the shared sin / cos / atan2: pose, flags, trace and currentChi have the restatement's bits"""
    assert same_bits(all_cases[key], pc.reference(key)), (key, all_cases[key]["trace"], pc.reference(key)["trace"])


@pytest.mark.parametrize("size", sorted(pc.BATCHES))
def test_batches_and_every_frame_alone(ctx, all_cases, size):
    keys = pc.BATCHES[size]
    got = run(ctx, keys)
    for k, g in zip(keys, got):
        check(k, g, pc.reference(k))
        assert same_bits(g, all_cases[k]), k                 # independent of what else is in the batch
        assert same_bits(run(ctx, [k])[0], g), k            # and of being alone
    assert all(same_bits(a, b) for a, b in zip(got, run(ctx, keys)))  # the same call twice


def test_pinned_inputs_give_the_same_bits(ctx, all_cases):
    keys = ["track_mixed_300_sparse", "kb8x2_63", "mono_2"]
    for k, g in zip(keys, run(ctx, keys, pinned=ctx)):
        assert same_bits(g, all_cases[k]), k


def test_flags_without_a_map_point_are_untouched(ctx):
    for key in ("track_mixed_300_sparse", "mixed_300_sparse", "mono_2", "mixed_no_points"):
        F = pc.ALL[key]
        g = run(ctx, [key], outlier=np.full(F["N"], 7, np.uint8))[0]
        has = F["has_point"].astype(bool)
        assert (g["outlier"][~has] == 7).all() and np.array_equal(g["outlier"][has], pc.reference(key)["outlier"][has])


def test_fewer_than_three_correspondences_return_zero_and_the_pose(ctx, all_cases):
    for key in ("mono_2", "mixed_no_points"):
        g, F = all_cases[key], pc.CASES[key]
        assert g["ret"] == 0 and np.array_equal(g["Tcw"][0], F["Tcw"][0]) and np.array_equal(g["Tcw"][1], F["Tcw"][1])
        assert g["trace"] == [(0, 0, 0.0)] * 4


def _call(ctx, frames, outliers):
    n = len(frames)
    Fa = (_capi.PoseOptFrame * n)(*frames)
    T = (_capi.SE3 * n)()
    O = (C.c_void_p * n)(*[None if o is None else _capi.ptr(o) for o in outliers])
    ret = np.full(n, -7, np.int32)
    return _capi.lib().ft_pose_optimization(ctx._h, n, Fa, T, O, _capi.ptr(ret), None), ret


def test_invalid_arguments_are_refused_without_a_launch(ctx):
    F = pc.CASES["kb8x2_63"]
    ok = pc.to_device(orb, pc.TRACKING["track_mono_100"])
    ctx.reset_stats()

    def variant(**change):
        d = pc.to_device(orb, F)
        keep.append(d)
        c = _capi.PoseOptFrame.from_buffer_copy(d.c)
        for k, v in change.items():
            setattr(c, k, v)
        return c

    keep = []
    Fm = dict(pc.TRACKING["track_mono_100"])
    Fm["keys"] = Fm["keys"].copy()
    Fm["keys"]["octave"][int(np.nonzero(Fm["has_point"])[0][0])] = pc.NLEVELS
    bad_octave = pc.to_device(orb, Fm)
    bad_q = variant()
    bad_q.Tcw.q[3] = 2.0
    cases = [bad_octave.c, variant(Nleft=F["N"] + 1), variant(world_pos=None), variant(has_point=None), variant(keys=None),
             variant(keys_right=None), variant(inv_level_sigma2=None), variant(nlevels=0), variant(cam_model=2), variant(N=-1), bad_q]
    for i, c in enumerate(cases):
        out = np.full(max(F["N"], 1), 7, np.uint8)
        rc, ret = _call(ctx, [ok.c, c], [ok.outlier, out])  # behind a valid frame: nothing of it is written either
        assert rc == _capi.FT_ERR_INVALID and (ret == -7).all() and (out == 7).all(), i
    rc, ret = _call(ctx, [ok.c], [None])
    assert rc == _capi.FT_ERR_INVALID
    big = pc.to_device(orb, pc.frame("mono", 3, _capi.POSE_OPT_MAX_EDGES + 1, noise=1.0))
    rc, ret = _call(ctx, [ok.c, big.c], [ok.outlier, big.outlier])
    assert rc == _capi.FT_ERR_CAPACITY and (ret == -7).all()
    assert ctx.get_stat("pose_optimization.launches")[1] == 0
    full = pc.frame("mono", 3, _capi.POSE_OPT_MAX_EDGES, noise=1.0, outliers=0.05)  # the capacity itself: 8 steps of 256 edges
    g = orb.pose_optimization(ctx, [pc.to_device(orb, full)])[0]
    assert ctx.get_stat("pose_optimization.launches") == (1.0, 1)
    assert same_bits(g, ref.pose_optimization(full)) and g["ret"] > 0.85 * _capi.POSE_OPT_MAX_EDGES

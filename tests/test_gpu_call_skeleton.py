"""The one-shot calls on the context's scratch (Arena + pinned mirror + CallScope, search_host.h) where the skeleton itself can
go wrong: a scratch that regrows in the middle of a call, one scratch reused by calls of different sizes, inputs the caller holds
in pinned memory, the vocabulary's own arena.  Every result equals the oracle's, no tolerance.  Needs an MI355X."""
import numpy as np
import pytest

from fasttrack_amd import orb, synth
from oracle import binding as ob
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

LOG_SF = float(np.float32(np.log(np.float32(1.2))))


@pytest.fixture()
def fresh_ctx():
    """a context whose scratch has not been allocated yet"""
    c = orb.Context(0)
    yield c
    c.close()


def _views(fr, sf, w, h, uright=None):
    args = dict(keys=fr["kL"], descriptors=fr["dL"], bounds=sc.frame_bounds(w, h), mbf=fr["intr"]["mbf"], mb=fr["intr"]["mb"],
                uright=uright, cam=[fr["intr"][k] for k in ("fx", "fy", "cx", "cy")])
    return ob.FrameView(scale_factors_=sf, **args), orb.FrameView(scale_factors=sf, **args)


def test_features_in_area_regrows_the_scratch_between_its_phases(fresh_ctx):
    """64 windows over the whole image of a 400-keypoint frame: the hit keys (64 x N x 4 bytes, ~100 KB) exceed the 1.5x headroom
    of the first allocation (the frame and the queries, ~30 KB), so the scratch is reallocated between the count and the write
    phase and the inputs go up again."""
    w, h = 640, 480
    fr = sc.oracle_stereo_frame(w, h, 400, 31)
    N = len(fr["kL"])
    assert 390 <= N < 512  # (the octree may return a few more than it was asked for)
    sf, _ = ob.scale_factors(1.2, 8)
    oF, gF = _views(fr, sf, w, h)
    nq = 64
    rng = np.random.default_rng(5)
    x = rng.uniform(0, w, nq).astype(np.float32)
    y = rng.uniform(0, h, nq).astype(np.float32)
    r = np.full(nq, 2000.0, np.float32)
    lo = np.full(nq, -1, np.int32)
    hi = np.full(nq, -1, np.int32)
    got, cnt = orb.features_in_area(fresh_ctx, gF, x, y, r, lo, hi, None, capacity=512)
    for q in range(nq):
        o = ob.features_in_area(oF, float(x[q]), float(y[q]), 2000.0, -1, -1, False)
        assert len(o) == N and cnt[q] == N and np.array_equal(got[q], o), q
    # the same context again, nothing regrows: same answer
    got2, cnt2 = orb.features_in_area(fresh_ctx, gF, x, y, r, lo, hi, None, capacity=512)
    assert np.array_equal(cnt2, cnt) and all(np.array_equal(a, b) for a, b in zip(got, got2))


def test_mixed_calls_share_one_scratch(fresh_ctx):
    """seven calls on one fresh context, each laying the scratch out anew at another size (growing and not growing)"""
    ctx = fresh_ctx
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, (5000, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (5000, 32), dtype=np.uint8)
    b[:2] = a[:2]

    def distance(n):
        g = orb.KernelController.descriptor_distance(ctx, a[:n], b[:n])
        assert np.array_equal(g, [ob.descriptor_distance(a[i], b[i]) for i in range(n)]), n

    voc = synth.make_vocabulary(10, 3, seed=5)
    ov = ob.Vocabulary(10, 3, 0, 0, voc["parent"], voc["is_leaf"], voc["descriptors"], voc["weights"])
    S = sc.bow_match_scenario(voc, ov.transform, 300, 700, 4, two_cam=False, levelsup=2)
    side = lambda d: orb.BowSide(d["fv_nodes"], d["fv_offsets"], d["fv_features"], d["descriptors"], d["angles"])  # noqa: E731
    w, h = 640, 480
    fr = sc.oracle_stereo_frame(w, h, 500, 33)
    sf, _ = ob.scale_factors(1.2, 8)
    sm = ob.stereo_match(fr["exL"], fr["exR"], fr["kL"], fr["kR"], fr["dL"], fr["dR"], fr["intr"]["mbf"], fr["intr"]["mb"])
    pts, Rcw, tcw = sc.map_points_scenario(fr["kL"], fr["dL"], sm["depth"], fr["intr"], 8, sf, 77, M=50)
    oF, gF = _views(fr, sf, w, h, uright=sm["uright"])
    R = sc.fisheye_rig_scenario(13, n=200)
    n = len(R["xy1"])
    dL = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    perm = rng.permutation(n)
    dR = dL[perm].copy()
    dR[:, 0] ^= 1
    kL = np.zeros(n, ob.KP_DTYPE); kR = np.zeros(n, ob.KP_DTYPE)
    kL["x"], kL["y"], kL["octave"] = R["xy1"][:, 0], R["xy1"][:, 1], R["octave1"]
    kR["x"], kR["y"], kR["octave"] = R["xy2"][perm, 0], R["xy2"][perm, 1], R["octave2"][perm]
    ls2 = (sf ** 2).astype(np.float32)

    distance(3)
    for ori in (True, False):
        o = ob.search_by_bow(S["kf"], S["has_point"], S["f"], S["nleft"], 0.7, ori)
        g = orb.search_by_bow(ctx, side(S["kf"]), S["has_point"], side(S["f"]), S["nleft"], 0.7, ori)
        assert o["n"] > 50 and g["n"] == o["n"] and np.array_equal(g["matches"], o["matches"]), ori
    o = ob.fisheye_match(a[:64], b[:65])
    g = orb.KernelController.launchFisheyeStereoMatchKernel(ctx, a[:64], b[:65])
    assert all(np.array_equal(g[k], o[k]) for k in ("matches", "best", "second"))
    o = ob.is_in_frustum(oF, ob.make_pose(Rcw, tcw), pts, 0.5, LOG_SF)
    g = orb.is_in_frustum(ctx, gF, orb.make_pose(Rcw, tcw), pts, 0.5, LOG_SF)
    assert 0 < o["n"] < 50 and g["n"] == o["n"]
    for k, _ in ob.FRUSTUM_FIELDS:
        assert np.array_equal(g[k], o[k]), k
    distance(5000)
    o = ob.fisheye_stereo(ob.make_rig(sc.KB8_CAM, sc.KB8_CAM, R["Rlr"], R["tlr"]), dL, kL, dR, kR, ls2)
    g = orb.fisheye_stereo(ctx, sc.KB8_CAM, sc.KB8_CAM, R["Rlr"], R["tlr"], dL, kL, dR, kR, ls2)
    assert o["n"] > 50 and g["n"] == o["n"] and np.array_equal(g["matches"], o["matches"])
    assert np.array_equal(g["depth"], o["depth"]) and np.array_equal(g["p3d"], o["p3d"])
    distance(3)


def test_fisheye_match_reads_pinned_descriptors_in_place(fresh_ctx):
    """descriptors in ft_host_malloc memory go up from where they are: byte-equal to the pageable call, either side or both"""
    ctx = fresh_ctx
    rng = np.random.default_rng(17)
    dL = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    pL = ctx.pinned_array((64, 32), np.uint8)
    pL[...] = dL
    for nR in (65, 1, 0):
        dR = rng.integers(0, 256, (nR, 32), dtype=np.uint8)
        dR[: nR // 2] = dL[: nR // 2]
        pR = ctx.pinned_array((nR, 32), np.uint8)
        pR[...] = dR
        want = orb.KernelController.launchFisheyeStereoMatchKernel(ctx, dL, dR)
        o = ob.fisheye_match(dL, dR)
        assert np.array_equal(want["matches"], o["matches"])
        if nR >= 2:
            assert np.array_equal(want["best"], o["best"]) and np.array_equal(want["second"], o["second"])
        for left, right in ((pL, pR), (pL, dR), (dL, pR)):
            g = orb.KernelController.launchFisheyeStereoMatchKernel(ctx, left, right)
            for k in ("matches", "best", "second"):
                assert g[k].tobytes() == want[k].tobytes(), (nR, k)


def test_bow_transform_arena_regrows_and_reads_resident_descriptors(fresh_ctx):
    """one vocabulary: 50 features, then 3 000 (its arena and the pinned mirror regrow together), then descriptors that are
    resident on the device (no copy up), then a single feature"""
    ctx = fresh_ctx
    voc = synth.make_vocabulary(10, 4, seed=9)
    args = (voc["parent"], voc["is_leaf"], voc["descriptors"], voc["weights"])
    gv, ov = orb.Vocabulary(ctx, 10, 4, 0, 0, *args), ob.Vocabulary(10, 4, 0, 0, *args)
    rng = np.random.default_rng(23)

    def same(want, got):
        for k in want:
            assert np.array_equal(want[k], got[k]), k

    for n in (50, 3000):
        d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        d[: n // 3] = voc["descriptors"][rng.integers(1, len(voc["parent"]), n // 3)]
        same(ov.transform(d, 2), gv.transform(d, 2))
    w, h = 640, 480
    intr = synth.intrinsics(w, h)
    fe = orb.StereoFrontend(ctx, 1000, 1.2, 8, 20, 7, w, h, 1, intr["mbf"], intr["mb"])
    L, R = synth.make_stereo_pair(w, h, 7)[:2]
    out = fe.process([L], [R])[0]
    want = ov.transform(out["descL"], 4)
    assert len(want["bow_ids"]) > 100
    same(want, gv.transform(None, 4, device_ptr=fe.device_descriptors(0), n=len(out["descL"])))
    same(ov.transform(out["descL"][:1], 4), gv.transform(None, 4, device_ptr=fe.device_descriptors(0), n=1))
    same(ov.transform(d[:1], 2), gv.transform(d[:1], 2))
    fe.close()
    gv.close()

"""-m gpu: ft_tracked_batch_* on frames beyond the LDS last-writer tables.  k_resolve_batch keeps its per-keypoint table in LDS up
to 12 288 keypoints of the batch's largest frame and in HBM beyond, k_replay_batch up to 15 360 (csrc/tracked_batch.cpp): the
regimes of tests/batch_large_cases.py sit on both sides of both thresholds, so every instantiation of the two kernels runs -
the HBM ones on the small frames of the batch as well.  Every search goes through the C ABI and is compared with the oracle's
sequence on the frame, field by field as in test_gpu_batch.py.  A mismatch is a finding: nothing here retries."""
import numpy as np
import pytest

from fasttrack_amd import orb
from tests import batch_large_cases as bc
from tests import scenarios as sc
from tests.test_gpu_batch import _check_frame

pytestmark = pytest.mark.gpu

MAX_POINTS = 512


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def _batch_inputs(case):
    """device views and call arguments of a regime's frames (the views are fresh: holder_obs starts as the case says)"""
    views = [orb.FrameView(scale_factors=bc.scale_factors(), **bc.frame_kw(f["a"])) for f in case]
    lasts, Tcws = [f["inputs"][0] for f in case], [f["inputs"][1] for f in case]
    ptss = [f["inputs"][2] for f in case]
    poses = [orb.make_pose(f["inputs"][3], f["inputs"][4], sc.KB8_TLR) for f in case]
    return views, lasts, Tcws, ptss, poses


def _searches(tb, views, lasts, Tcws, ptss, poses):
    """upload, SearchByProjection(CurrentFrame, LastFrame) with the rotation filter, isInFrustum + the local-map search"""
    tb.upload(views)
    g1 = tb.search_last_frame(lasts, Tcws, bc.TH, check_orientation=True)
    g2 = tb.track_local_map(poses, ptss, 0.5, bc.LOG_SF, bc.TH)
    return g1, g2, [tb.holder_obs(f) for f in range(len(views))]


def _check_case(tag, case, g1, g2, gh):
    for f, fr in enumerate(case):
        _check_frame(f"{tag} {fr['which']} frame", g1[f], g2[f], gh[f], *fr["oracle"])


def _same(a, b):
    (a1, a2, ah), (b1, b2, bh) = a, b
    return all(x["n"] == y["n"] and np.array_equal(x["assign"], y["assign"]) for x, y in zip(a1 + a2, b1 + b2)) and \
        all(x["n_to_match"] == y["n_to_match"] for x, y in zip(a2, b2)) and all(np.array_equal(x, y) for x, y in zip(ah, bh))


def _fallbacks(ctx):
    try:
        return ctx.get_stat("tracked_batch.resolve_fallbacks")[1]
    except orb.FastTrackError:
        return 0   # (a series nobody added to since the reset)


@pytest.mark.parametrize("n_total", bc.REGIMES)
def test_every_table_regime_resolves_to_the_oracles_results(ctx, n_total):
    """search_cache 3, the plain points: every frame of the batch equals the oracle; k_resolve_batch gave up on no frame (the
    resolution produced the results, not the claim passes); and the two small frames uploaded alone - both tables in LDS - get
    exactly the arrays they got beside the large frame"""
    case = bc.regime_case(n_total, "plain")
    args = _batch_inputs(case)
    with ctx.options(search_cache=3):
        tb = orb.TrackedBatch(ctx, max_frames=3, max_keypoints=n_total + 8, max_points=MAX_POINTS)
        try:
            ctx.reset_stats()
            beside = _searches(tb, *args)
            assert _fallbacks(ctx) == 0
            _check_case(f"{n_total}", case, *beside)
            alone = _searches(tb, *[x[1:] for x in _batch_inputs(case)])
            assert _fallbacks(ctx) == 0
            assert _same(alone, tuple(x[1:] for x in beside))
        finally:
            tb.close()


@pytest.mark.parametrize("pattern", list(bc.PATTERNS))
@pytest.mark.parametrize("n_total", bc.REGIMES)
def test_chunk_hand_over_in_every_table_regime(ctx, n_total, pattern):
    """the directed cases: copies of 40 points, one per 64-point chunk of k_resolve_batch's walk, whose Observations() follow a
    pattern per chunk - a copy's result depends on the last writers the chunks in front of it published (the table in LDS or in
    HBM), the final assignment on k_replay_batch's table; last-frame search (rotation filter on) and local-map search"""
    case = bc.regime_case(n_total, pattern)
    with ctx.options(search_cache=3):
        tb = orb.TrackedBatch(ctx, max_frames=3, max_keypoints=n_total + 8, max_points=MAX_POINTS)
        try:
            ctx.reset_stats()
            got = _searches(tb, *_batch_inputs(case))
            assert _fallbacks(ctx) == 0
            _check_case(f"{n_total} {pattern}", case, *got)
        finally:
            tb.close()


@pytest.mark.parametrize("n_total", [12289, 15361])
def test_claim_passes_on_the_large_tables(ctx, n_total):
    """search_cache 1, bursts of two passes: the claim passes run on the writer tables of a large passK(N), and k_replay_batch
    (its table in LDS at 12 289, in HBM at 15 361) runs behind every burst with a flag position"""
    case = bc.regime_case(n_total, "alternate")
    with ctx.options(search_cache=1, pass_burst=2):
        tb = orb.TrackedBatch(ctx, max_frames=3, max_keypoints=n_total + 8, max_points=MAX_POINTS)
        try:
            _check_case(f"{n_total} passes", case, *_searches(tb, *_batch_inputs(case)))
        finally:
            tb.close()


def test_submit_and_wait_with_pinned_arrays_on_the_largest_regime(ctx):
    """15 361 keypoints through ft_tracked_batch_submit_* / _wait, point and assignment arrays pinned: k_replay_batch<*, false>
    writes `assign` straight into pinned host memory.  The same results as the blocking calls (and as the oracle)."""
    n_total = 15361
    case = bc.regime_case(n_total, "alternate")
    with ctx.options(search_cache=3):
        tb = orb.TrackedBatch(ctx, max_frames=3, max_keypoints=n_total + 8, max_points=MAX_POINTS, pinned=True)
        try:
            views, lasts, Tcws, ptss, poses = _batch_inputs(case)
            pl_last, pl_local = tb.prepare_last(lasts, Tcws, ctx=ctx), tb.prepare_local(poses, ptss, ctx=ctx)
            tb.upload(views)
            assert tb.search_last_frame(pl_last, th=bc.TH, submit=True) is None
            g1 = tb.wait()
            assert tb.track_local_map(pl_local, viewing_cos_limit=0.5, log_scale_factor=bc.LOG_SF, th=bc.TH, submit=True) is None
            g2 = tb.wait()
            split = (g1, g2, [tb.holder_obs(f) for f in range(3)])
            _check_case("submit + wait", case, *split)
            views = _batch_inputs(case)[0]
            tb.upload(views)
            b1 = tb.search_last_frame(pl_last, th=bc.TH)
            b2 = tb.track_local_map(pl_local, viewing_cos_limit=0.5, log_scale_factor=bc.LOG_SF, th=bc.TH)
            assert _same(split, (b1, b2, [tb.holder_obs(f) for f in range(3)]))
            for f in range(3):   # (the frustum fields too)
                for k, _ in bc.ob.FRUSTUM_FIELDS:
                    assert np.array_equal(g2[f][k], b2[f][k]), (f, k)
        finally:
            tb.close()


def test_single_frame_path_on_the_largest_padded_frame(ctx):
    """the padded frame of 15 361 keypoints (30 % of them held before the call) through ft_tracked_frame_*: the same assignments
    and holder_obs as the batch gives it"""
    n_total = 15361
    case = bc.regime_case(n_total, "alternate")
    views, lasts, Tcws, ptss, poses = _batch_inputs(case)
    with ctx.options(search_cache=3):
        tb = orb.TrackedBatch(ctx, max_frames=3, max_keypoints=n_total + 8, max_points=MAX_POINTS)
        tf = orb.TrackedFrame(ctx, max_keypoints=n_total + 8, max_points=MAX_POINTS)
        try:
            g1, g2, gh = _searches(tb, views, lasts, Tcws, ptss, poses)
            tf.upload(_batch_inputs(case)[0][0])
            s1 = tf.search_last_frame(lasts[0], Tcws[0], bc.TH)
            s2 = tf.track_local_map(poses[0], ptss[0], 0.5, bc.LOG_SF, bc.TH)
            _check_frame("single-frame path", s1, s2, tf.holder_obs(), *case[0]["oracle"])
            assert s1["n"] == g1[0]["n"] and np.array_equal(s1["assign"], g1[0]["assign"])
            assert s2["n"] == g2[0]["n"] and np.array_equal(s2["assign"], g2[0]["assign"]) and s2["n_to_match"] == g2[0]["n_to_match"]
            assert np.array_equal(tf.holder_obs(), gh[0])
        finally:
            tf.close()
            tb.close()


@pytest.mark.parametrize("n_total", [12289, 15361])
def test_large_frames_give_the_same_results_every_time(ctx, n_total):
    """upload + both searches four times over through one batch object: every run identical to the first (which is the oracle's)"""
    case = bc.regime_case(n_total, "all3")
    with ctx.options(search_cache=3):
        tb = orb.TrackedBatch(ctx, max_frames=3, max_keypoints=n_total + 8, max_points=MAX_POINTS)
        try:
            first = _searches(tb, *_batch_inputs(case))
            _check_case(f"{n_total} run 0", case, *first)
            for rep in range(1, 4):
                assert _same(_searches(tb, *_batch_inputs(case)), first), f"{n_total}: run {rep} differs from run 0"
        finally:
            tb.close()

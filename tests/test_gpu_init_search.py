"""ft_search_for_initialization / ft_tracked_frame_search_for_initialization against the restatement of
ORBmatcher::SearchForInitialization (tests/init_search_ref.py), bit for bit: vnMatches12, vbPrevMatched (float32 bits),
nmatches, vMatchedDistance.  Needs an MI355X.

What the restatement reports on the inputs used here (window 100, ratio 0.9, orientation check on; frames extracted by the
library's extractor with the mono lapping area (0, 1000); "level 0" = keypoints of F1 with octave 0):
  752x480  seed 3 rolled (4, 12)   nFeatures 5000: 3398 / 3593 keypoints, 673 level 0, 55695 candidates, 560 accepted,
                                   33 evictions, 20134 skipped, 7 removed by the histogram, 28 evicted in kept bins, n 520
  752x480  seed 4 rolled (13, 40)  nFeatures 5000: 637 level 0, 460 accepted, 30 evictions, 16868 skipped, n 422
  640x480  seed 5 rolled (8, 25)   nFeatures 5000: 559 level 0, 471 accepted, 47 evictions, 15235 skipped, n 415
  1280x720 seed 6 rolled (20, 55)  nFeatures 10000: 8909 / 9173 keypoints, 1703 level 0, 1230 accepted, 71 evictions, n 1140
  1280x720 mosaic seed 11          nFeatures 10000: 10008 / 10009 keypoints, 2172 level 0, 196529 candidates, n 666
  dictionary descriptors (752x480 seed 3's keypoints), seeds 1 - 4: 65 / 74 / 16 / 148 evictions, 391 / 302 / 542 / 52 ratio
                                   failures, 150 / 186 / 69 / 217 removed by the histogram; the evicted entries change which bins
                                   survive for seeds 1, 2, 4
(the synthetic scenes give about 3400 keypoints for a quota of 5000: the generator, not a fault.)
The non-vacuity test asserts the conditions themselves (evictions, skipped candidates, histogram removals, an evicted entry
in a surviving bin, n_matches >= 100 on every real-frame case) on the restatement's side."""
import threading

import numpy as np
import pytest

from fasttrack_amd import orb, synth
from oracle import binding as ob
from tests import init_search_ref as ref
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

SF, _ = ob.scale_factors(1.2, 8)
LAP = (0, 1000)


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def displaced(img, dx, dy, seed):
    """the same scene moved by (dx, dy) pixels, with fresh noise of +-3"""
    rng = np.random.default_rng(1000 + seed)
    moved = np.roll(img, (dy, dx), axis=(0, 1)).astype(np.int32) + rng.integers(-3, 4, img.shape)
    return np.ascontiguousarray(np.clip(moved, 0, 255).astype(np.uint8))


_frames = {}


def extract(ctx, w, h, nf, img_key, make):
    key = (w, h, nf, img_key)
    if key not in _frames:
        ex = orb.ORBextractor(ctx, nf, 1.2, 8, 20, 7, w, h)
        try:
            k, d, _ = ex(make(), LAP)
        finally:
            ex.close()
        _frames[key] = (k, d)
    return _frames[key]


def views(k, d, w, h):
    return ob.FrameView(k, d, SF, sc.frame_bounds(w, h)), orb.FrameView(k, d, SF, sc.frame_bounds(w, h))


def real_pair(ctx, w, h, nf, seed, dx, dy):
    base = lambda: synth.make_image(w, h, seed)
    k1, d1 = extract(ctx, w, h, nf, ("base", seed), base)
    k2, d2 = extract(ctx, w, h, nf, ("moved", seed, dx, dy), lambda: displaced(base(), dx, dy, seed))
    return k1, d1, k2, d2


def prev_of(k1):
    return np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def check_against_ref(tag, g, o, with_distance=True):
    assert g["n"] == o["n"], f"{tag}: n_matches {g['n']} != {o['n']}"
    assert np.array_equal(g["matches12"], o["matches12"]), f"{tag}: matches12"
    assert same_bits(g["prev_matched"], o["prev_matched"]), f"{tag}: prev_matched"
    if with_distance:
        assert np.array_equal(g["matched_distance"], o["matched_distance"]), f"{tag}: matched_distance"


def run_both(ctx, k1, d1, k2, d2, w, h, prev, window, ratio, ori):
    """the restatement, the non-resident entry and the resident entry on one pair"""
    o2, g2 = views(k2, d2, w, h)
    _, g1 = views(k1, d1, w, h)
    o = ref.search_for_initialization(k1, d1, o2, prev, window, ratio, ori)
    g = orb.KernelController.search_for_initialization(ctx, g1, g2, prev, window, ratio, ori)
    ini = orb.TrackedFrame(ctx, max(len(k1), 1), 1)
    cur = orb.TrackedFrame(ctx, max(len(k2), 1), 1)
    try:
        ini.upload(g1)
        cur.upload(g2)
        t = cur.search_for_initialization(ini, prev, window, ratio, ori)
    finally:
        ini.close()
        cur.close()
    return o, g, t


REAL = [(752, 480, 5000, 3, 4, 12), (752, 480, 5000, 4, 13, 40), (640, 480, 5000, 5, 8, 25), (1280, 720, 10000, 6, 20, 55)]
_ref_stats = {}


@pytest.mark.parametrize("w,h,nf,seed,dx,dy", REAL)
@pytest.mark.parametrize("window,ratio,ori", [(100, 0.9, True), (100, 0.6, False), (100, 0.9, False)])
def test_real_frames(ctx, w, h, nf, seed, dx, dy, window, ratio, ori):
    k1, d1, k2, d2 = real_pair(ctx, w, h, nf, seed, dx, dy)
    o, g, t = run_both(ctx, k1, d1, k2, d2, w, h, prev_of(k1), window, ratio, ori)
    print(f"init_search {w}x{h} seed {seed} window {window} ratio {ratio} ori {ori}: N1 {len(k1)} N2 {len(k2)} n {o['n']} {o['stats']}")
    _ref_stats[(w, h, seed, window, ratio, ori)] = (o["n"], o["stats"])
    check_against_ref("non-resident", g, o)
    check_against_ref("resident", t, o, with_distance=False)
    assert o["n"] >= 100   # the reference's own bar for going on (src/Tracking.cc:2552)


def test_small_window(ctx):
    """window 15 around a displacement of (4, 12)"""
    w, h, nf, seed, dx, dy = REAL[0]
    k1, d1, k2, d2 = real_pair(ctx, w, h, nf, seed, dx, dy)
    for ori in (True, False):
        o, g, t = run_both(ctx, k1, d1, k2, d2, w, h, prev_of(k1), 15, 0.9, ori)
        print(f"init_search small window ori {ori}: n {o['n']} {o['stats']}")
        check_against_ref("non-resident", g, o)
        check_against_ref("resident", t, o, with_distance=False)
        assert o["n"] >= 100


def test_chained_as_tracking_chains_it(ctx):
    """Tracking::MonocularInitialization: one initial frame against successive current frames, every call's vbPrevMatched
    fed into the next (src/Tracking.cc:2516-2549).  Resident form = the restatement chained the same way = the non-resident entry."""
    w, h, nf, seed = 752, 480, 5000, 3
    base = lambda: synth.make_image(w, h, seed)
    k1, d1 = extract(ctx, w, h, nf, ("base", seed), base)
    _, g1 = views(k1, d1, w, h)
    ini = orb.TrackedFrame(ctx, len(k1), 1)
    cur = orb.TrackedFrame(ctx, 6000, 1)
    try:
        ini.upload(g1)
        prev_o = prev_t = prev_g = prev_of(k1)
        for step, (dx, dy) in enumerate([(3, 8), (7, 18), (12, 30)]):
            k2, d2 = extract(ctx, w, h, nf, ("moved", seed, dx, dy), lambda: displaced(base(), dx, dy, seed))
            o2, g2 = views(k2, d2, w, h)
            o = ref.search_for_initialization(k1, d1, o2, prev_o, 100, 0.9, True)
            cur.upload(g2)
            t = cur.search_for_initialization(ini, prev_t, 100, 0.9, True)
            g = orb.KernelController.search_for_initialization(ctx, g1, g2, prev_g, 100, 0.9, True)
            print(f"init_search chained step {step}: n {o['n']} {o['stats']}")
            check_against_ref(f"step {step} resident", t, o, with_distance=False)
            check_against_ref(f"step {step} non-resident", g, o)
            assert o["n"] >= 100
            prev_o, prev_t, prev_g = o["prev_matched"], t["prev_matched"], g["prev_matched"]
        assert not same_bits(prev_o, prev_of(k1))
    finally:
        ini.close()
        cur.close()


def adversarial(k1, seed, words=12):
    """descriptors of both frames from a dictionary of `words` values with 0 - 3 bits flipped: ties, evictions and ratio
    failures everywhere; F2 = F1's keypoints moved by a few pixels and shuffled"""
    rng = np.random.default_rng(seed)
    dic = rng.integers(0, 256, (words, 32), dtype=np.uint8)
    # words 30 - 60 bits apart, so that distances around TH_LOW occur: every word = word 0 with 15 - 30 flipped bits
    for wd in range(1, words):
        dic[wd] = dic[0]
        for b in rng.choice(256, int(rng.integers(15, 31)), replace=False):
            dic[wd, b // 8] ^= 1 << (b % 8)

    def draw(n):
        d = dic[rng.integers(0, words, n)].copy()
        for i in range(n):
            for b in rng.choice(256, int(rng.integers(0, 4)), replace=False):
                d[i, b // 8] ^= 1 << (b % 8)
        return d

    n1 = len(k1)
    perm = rng.permutation(n1)[:max(n1 - 37, 1)]   # N2 != N1
    k2 = k1[perm].copy()
    k2["x"] += rng.integers(-6, 7, len(k2)).astype(np.float32)
    k2["y"] += rng.integers(-6, 7, len(k2)).astype(np.float32)
    k2["angle"] = np.where(rng.random(len(k2)) < 0.7, k2["angle"], rng.uniform(0, 360, len(k2))).astype(np.float32)
    return draw(n1), k2, draw(len(k2))


@pytest.mark.parametrize("seed,window,ratio", [(1, 100, 0.9), (2, 30, 0.9), (3, 100, 0.6), (4, 15, 1.0)])
def test_adversarial_descriptors(ctx, seed, window, ratio):
    w, h = 752, 480
    k1, _ = extract(ctx, w, h, 5000, ("base", 3), lambda: synth.make_image(w, h, 3))
    d1, k2, d2 = adversarial(k1, seed)
    o, g, t = run_both(ctx, k1, d1, k2, d2, w, h, prev_of(k1), window, ratio, True)
    print(f"init_search adversarial seed {seed}: n {o['n']} {o['stats']}")
    _ref_stats[("adv", seed)] = (o["n"], o["stats"])
    check_against_ref("non-resident", g, o)
    check_against_ref("resident", t, o, with_distance=False)
    assert o["stats"]["evictions"] > 0 and o["stats"]["skipped"] > 0 and o["stats"]["ratio_rejected"] > 0


def test_inputs_exercise_the_sequential_part(ctx):
    """non-vacuity, on the restatement's side: over the real-frame and adversarial cases it reports evictions, candidates
    skipped by vMatchedDistance <= dist, matches removed by the histogram and evicted entries in surviving bins"""
    w, h, nf, seed, dx, dy = REAL[0]
    k1, d1, k2, d2 = real_pair(ctx, w, h, nf, seed, dx, dy)
    o2, _ = views(k2, d2, w, h)
    stats = [ref.search_for_initialization(k1, d1, o2, prev_of(k1), 100, 0.9, True)["stats"]]
    kb, _ = extract(ctx, 752, 480, 5000, ("base", 3), lambda: synth.make_image(752, 480, 3))
    for s in (1, 2):
        da, ka2, da2 = adversarial(kb, s)
        oa2, _ = views(ka2, da2, 752, 480)
        stats.append(ref.search_for_initialization(kb, da, oa2, prev_of(kb), 100 if s == 1 else 30, 0.9, True)["stats"])
    print("init_search non-vacuity:", stats)
    assert stats[0]["evictions"] >= 1 and stats[0]["skipped"] >= 1
    for key in ("evictions", "skipped", "removed_by_histogram", "evicted_in_kept_bin"):
        assert sum(s[key] for s in stats) >= 1, key


def test_edge_cases(ctx):
    w, h = 752, 480
    k1, d1, k2, d2 = real_pair(ctx, *REAL[0])
    prev = prev_of(k1)
    # F1 without a level-0 keypoint, F2 without one
    hi1, hi2 = k1["octave"] > 0, k2["octave"] > 0
    for tag, (a, b, c, d) in dict(no_rows=(k1[hi1], d1[hi1], k2, d2), no_candidates=(k1, d1, k2[hi2], d2[hi2])).items():
        o, g, t = run_both(ctx, a, b, c, d, w, h, prev_of(a), 100, 0.9, True)
        assert o["n"] == 0
        check_against_ref(tag, g, o)
        check_against_ref(tag, t, o, with_distance=False)
    # a window that covers the whole image; N1 != N2 (cut frames)
    # (with the lapping area (0, 1000) every keypoint is filled in from the back: level 0 sits at the END of the arrays)
    for tag, (a, b, c, d, win) in dict(whole_image=(k1[-900:], d1[-900:], k2, d2, 2000),
                                       cut=(k1[-1500:], d1[-1500:], k2[:-150], d2[:-150], 100)).items():
        o, g, t = run_both(ctx, a, b, c, d, w, h, prev_of(a), win, 0.9, True)
        print(f"init_search {tag}: n {o['n']} {o['stats']}")
        assert o["stats"]["level0"] > 300 and o["n"] > 0
        check_against_ref(tag, g, o)
        check_against_ref(tag, t, o, with_distance=False)
    # vbPrevMatched outside the image bounds (left / above, right / below, and far away)
    rng = np.random.default_rng(9)
    out = prev.copy()
    sel = rng.random(len(out)) < 0.5
    out[sel] += rng.choice(np.array([-150.0, -60.0, 90.0, 800.0, 5000.0], np.float32), (int(sel.sum()), 2))
    o, g, t = run_both(ctx, k1, d1, k2, d2, w, h, out, 100, 0.9, True)
    print(f"init_search outside: n {o['n']} {o['stats']}")
    check_against_ref("outside", g, o)
    check_against_ref("outside", t, o, with_distance=False)
    # an empty F1 / F2
    e = np.zeros(0, ob.KP_DTYPE), np.zeros((0, 32), np.uint8)
    g = orb.KernelController.search_for_initialization(ctx, views(*e, w, h)[1], views(k2, d2, w, h)[1], np.zeros((0, 2), np.float32))
    assert g["n"] == 0 and len(g["matches12"]) == 0 and (g["matched_distance"] == ref.INT_MAX).all()
    g = orb.KernelController.search_for_initialization(ctx, views(k1, d1, w, h)[1], views(*e, w, h)[1], prev)
    assert g["n"] == 0 and (g["matches12"] == -1).all() and same_bits(g["prev_matched"], prev)


def test_invalid_arguments(ctx):
    w, h = 752, 480
    k1, d1, k2, d2 = real_pair(ctx, *REAL[0])
    g1, g2 = views(k1, d1, w, h)[1], views(k2, d2, w, h)[1]
    with pytest.raises(orb.FastTrackError) as e:
        orb.KernelController.search_for_initialization(ctx, g1, g2, prev_of(k1), window=0)
    assert e.value.status == -1
    two = orb.FrameView(k2[:10], np.concatenate([d2[:10], d2[:5]]), SF, sc.frame_bounds(w, h), keys_right=k2[:5],
                        left_to_right=np.full(10, -1, np.int32), right_to_left=np.full(5, -1, np.int32))
    with pytest.raises(orb.FastTrackError) as e:
        orb.KernelController.search_for_initialization(ctx, g1, two, prev_of(k1))
    assert e.value.status == -1


def test_ten_thousand_keypoints(ctx):
    """the 5 x nFeatures frame of the initialisation extractor at nFeatures 2000, on a dense scene that fills the quota"""
    w, h, nf = 1280, 720, 10000
    L, R = synth.make_mosaic_pair(w, h, 11, block=8, disparity=9)
    k1, d1 = extract(ctx, w, h, nf, ("mosaicL", 11), lambda: L)
    k2, d2 = extract(ctx, w, h, nf, ("mosaicR", 11), lambda: R)
    assert len(k1) >= 9500 and len(k2) >= 9500
    o, g, t = run_both(ctx, k1, d1, k2, d2, w, h, prev_of(k1), 100, 0.9, True)
    print(f"init_search 10k: N1 {len(k1)} N2 {len(k2)} n {o['n']} {o['stats']}")
    check_against_ref("non-resident", g, o)
    check_against_ref("resident", t, o, with_distance=False)


def test_launch_count_is_fixed(ctx):
    """three kernels per resident call whatever the frames hold (four for the non-resident entry: it builds F2's grid)"""
    w, h = 752, 480
    k1, d1, k2, d2 = real_pair(ctx, *REAL[0])
    g1, g2 = views(k1, d1, w, h)[1], views(k2, d2, w, h)[1]
    small1, small2 = views(k1[-40:], d1[-40:], w, h)[1], views(k2[-25:], d2[-25:], w, h)[1]   # (level 0 sits at the end)
    ini, cur = orb.TrackedFrame(ctx, len(k1), 1), orb.TrackedFrame(ctx, len(k2), 1)
    try:
        ctx.set_kernel_timing(True)
        ctx.reset_stats()
        calls = 0
        for a, b, win in ((g1, g2, 100), (small1, g2, 100), (g1, small2, 15), (g1, g2, 2000)):
            ini.upload(a)
            cur.upload(b)
            cur.search_for_initialization(ini, prev_of(a.keys), win)
            calls += 1
            assert ctx.get_stat("tracked.search_for_initialization.launches") == (3.0 * calls, calls)
        for name in ("kernel.init_prepare", "kernel.init_candidates", "kernel.init_resolve"):
            assert ctx.get_stat(name)[1] == calls, name
        orb.KernelController.search_for_initialization(ctx, g1, g2, prev_of(k1))
        assert ctx.get_stat("search_for_initialization.launches") == (4.0, 1)
        assert ctx.get_stat("kernel.init_resolve")[1] == calls + 1
    finally:
        ctx.set_kernel_timing(False)
        ini.close()
        cur.close()


def test_two_contexts_from_two_threads(ctx):
    """the entry points are re-entrant across handles: two contexts, two host threads, equal results"""
    w, h = 752, 480
    k1, d1, k2, d2 = real_pair(ctx, *REAL[0])
    prev = prev_of(k1)
    o = ref.search_for_initialization(k1, d1, views(k2, d2, w, h)[0], prev, 100, 0.9, True)
    other = orb.Context(0)
    results, errors = {}, []

    def work(c, tag):
        try:
            g1, g2 = views(k1, d1, w, h)[1], views(k2, d2, w, h)[1]
            ini, cur = orb.TrackedFrame(c, len(k1), 1), orb.TrackedFrame(c, len(k2), 1)
            try:
                ini.upload(g1)
                cur.upload(g2)
                for rep in range(8):
                    results[(tag, rep, "t")] = cur.search_for_initialization(ini, prev)
                    results[(tag, rep, "g")] = orb.KernelController.search_for_initialization(c, g1, g2, prev)
            finally:
                ini.close()
                cur.close()
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    try:
        ths = [threading.Thread(target=work, args=(c, tag)) for c, tag in ((ctx, "a"), (other, "b"))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    finally:
        other.close()
    assert not errors, errors
    assert len(results) == 32
    for key, r in results.items():
        check_against_ref(str(key), r, o, with_distance=key[2] == "g")

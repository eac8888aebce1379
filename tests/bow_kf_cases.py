"""Inputs of ORBmatcher::SearchByBoW(KeyFrame, KeyFrame) for the tests of ft_search_by_bow_keyframes: scenarios of one keyframe 1
with J neighbours, single-node cases of a given size, and hand-built cases whose expected outputs are written out from the
reference text (src/ORBmatcher.cc:864-1004).  Keyframes are the dicts tests/bow_kf_ref.py takes; to_device() turns one into the
library's BowKeyFrame.

The descriptors follow the recipe of fasttrack_amd.scenarios.bow_match_scenario: keyframe-1 descriptors sit near vocabulary
centres; most descriptors of a neighbour are keyframe-1 descriptors with 0 - 14 flipped bits (several copies of the same one: equal
distances, failed ratio tests, claims), some are 40 - 60 bits away (around TH_LOW), the rest random, a tenth are exact copies of
another descriptor of the same neighbour; the angles follow one dominant rotation per neighbour with outliers.  The FeatureVectors
come from a synthetic vocabulary (fasttrack_amd.synth.make_vocabulary) through the oracle's transform.
"""
import functools

import numpy as np

from fasttrack_amd import scenarios as fsc
from fasttrack_amd import synth
from oracle import binding as ob

f32 = np.float32


@functools.lru_cache(maxsize=None)
def vocabulary(k=10, L=4, seed=17):
    """-> (synth dict, oracle Vocabulary)"""
    v = synth.make_vocabulary(k, L, seed)
    return v, ob.Vocabulary(k=v["k"], L=v["L"], parent=v["parent"], is_leaf=v["is_leaf"], descriptors=v["descriptors"], weights=v["weights"])


def keyframe(fv, descriptors, angles, has_point, n_left=-1, n_un=None):
    d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
    return dict(fv_nodes=np.asarray(fv["fv_nodes"], np.uint32), fv_offsets=np.asarray(fv["fv_offsets"], np.int32),
                fv_features=np.asarray(fv["fv_features"], np.uint32), descriptors=d, angles=np.asarray(angles, f32),
                has_point=np.asarray(has_point, np.uint8), n_left=int(n_left), n_un=len(d) if n_un is None else int(n_un))


def _near(rng, base, lo, hi):
    out = np.array(base, np.uint8).reshape(-1, 32).copy()
    for i in range(len(out)):
        nb = int(rng.integers(lo, hi + 1))
        if nb:
            bits = np.unpackbits(out[i])
            bits[rng.choice(256, nb, replace=False)] ^= 1
            out[i] = np.packbits(bits)
    return out


def _neighbour_descriptors(rng, d1, a1, src_pool, n2):
    """n2 descriptors and angles derived from keyframe 1 (d1, a1); src_pool: the keyframe-1 features a copy may come from"""
    src = src_pool[rng.integers(0, len(src_pool), n2)]
    kind = rng.random(n2)
    d2 = np.zeros((n2, 32), np.uint8)
    close, mid, rnd = kind < 0.7, (kind >= 0.7) & (kind < 0.85), kind >= 0.85
    d2[close] = _near(rng, d1[src[close]], 0, 14)
    d2[mid] = _near(rng, d1[src[mid]], 40, 60)
    d2[rnd] = rng.integers(0, 256, (int(rnd.sum()), 32), dtype=np.uint8)
    dup = rng.random(n2) < 0.1  # exact copies of another descriptor of this neighbour: ties in scan order
    d2[dup] = d2[rng.integers(0, n2, int(dup.sum()))]
    rot = f32(rng.uniform(0, 360))
    a2 = (a1[src] - rot + rng.normal(0, 4, n2)).astype(f32)
    outl = rng.random(n2) < 0.2
    a2[outl] = rng.uniform(0, 360, int(outl.sum()))
    return d2, np.mod(a2, f32(360)).astype(f32)


@functools.lru_cache(maxsize=None)
def scenario(seed, n1=500, n2=(400, 500, 600), levelsup=2, two_cam=False, empty_neighbour=False, pointless_neighbour=False,
             foreign_neighbour=False, vocab=(10, 4, 17), has1=0.8, has2=0.6):
    """keyframe 1 with n1 features against len(n2) neighbours -> dict(kf1, neighbours).  two_cam: every keyframe has two cameras,
    n_un = n_left ~ 0.55 n, and its FeatureVector lists the right camera's features as well.  empty_neighbour /
    pointless_neighbour / foreign_neighbour: one more neighbour with no feature / without a map point / with features of other
    vocabulary nodes only."""
    rng = np.random.default_rng(seed)
    voc, ovoc = vocabulary(*vocab)
    centres = voc["descriptors"][1:]
    d1 = _near(rng, centres[rng.integers(0, len(centres), n1)], 0, 20)
    a1 = rng.uniform(0, 360, n1).astype(f32)
    nl1 = int(n1 * 0.55) if two_cam else -1
    kf1 = keyframe(ovoc.transform(d1, levelsup), d1, a1, rng.random(n1) < has1, nl1, nl1 if two_cam else None)
    pool = np.arange(nl1 if two_cam else n1)  # a neighbour copies the features keyframe 1 can match
    kfs = []
    for m in n2:
        d2, a2 = _neighbour_descriptors(rng, d1, a1, pool, m)
        nl2 = int(m * 0.55) if two_cam else -1
        kfs.append(keyframe(ovoc.transform(d2, levelsup), d2, a2, rng.random(m) < has2, nl2, nl2 if two_cam else None))
    if empty_neighbour:
        kfs.insert(1, keyframe(dict(fv_nodes=[], fv_offsets=[0], fv_features=[]), np.zeros((0, 32), np.uint8), [], [], 0 if two_cam else -1, 0))
    if pointless_neighbour:
        kfs.insert(3, dict(kfs[0], has_point=np.zeros_like(kfs[0]["has_point"])))
    if foreign_neighbour:
        kfs.append(dict(kfs[0], fv_nodes=(kfs[0]["fv_nodes"] + np.uint32(100000)).astype(np.uint32)))
    return dict(kf1=kf1, neighbours=kfs)


# The scenarios the CPU and the GPU tests share, (seed, keyword arguments): ~100 nodes, ~10 nodes and one node (700 x 700: the path of
# the lists too long for the registers), one and two cameras.  test_bow_kf_cpu.py asserts that none of them is vacuous.
MAIN = [(41, dict(levelsup=2)), (42, dict(levelsup=2, two_cam=True, n1=700, n2=(600, 700, 650))), (43, dict(levelsup=3)),
        (44, dict(levelsup=3, two_cam=True, n1=700, n2=(600, 700, 650))), (45, dict(levelsup=4, n1=700, n2=(700, 700, 700)))]
CONFIGS = [(0.9, True), (0.7, False), (0.6, True)]  # (nn_ratio, check_orientation)


def main_scenario(i):
    seed, kw = MAIN[i]
    return scenario(seed, **kw)


def oracle_pair(n_kf, n_f, levelsup, seed):
    """scenarios.bow_match_scenario as the pair (keyframe 1, keyframe 2) with one camera and every keyframe-2 feature holding a
    point, next to the oracle's own inputs -> (S, kf1, kf2)"""
    voc, ovoc = vocabulary(10, 4, 17)
    S = fsc.bow_match_scenario(voc, ovoc.transform, n_kf, n_f, seed, levelsup=levelsup)
    kf1 = keyframe(S["kf"], S["kf"]["descriptors"], S["kf"]["angles"], S["has_point"])
    kf2 = keyframe(S["f"], S["f"]["descriptors"], S["f"]["angles"], np.ones(n_f, np.uint8))
    return S, kf1, kf2


ORACLE_PAIRS = [(300, 400, 2, 0), (500, 300, 3, 1), (200, 200, 4, 2), (64, 65, 1, 3), (700, 600, 2, 4), (257, 300, 4, 5)]


def one_node(order, node=0):
    order = np.asarray(order, np.uint32)
    return dict(fv_nodes=np.array([node], np.uint32), fv_offsets=np.array([0, len(order)], np.int32), fv_features=order)


@functools.lru_cache(maxsize=None)
def node_size_case(k1, k2, seed=0, extra1=3, extra2=0):
    """ONE shared node with exactly k1 eligible keyframe-1 features and k2 eligible candidates; extra1 / extra2 more features of
    the node's lists hold no map point.  The lists are in shuffled order."""
    rng = np.random.default_rng(1000 * k1 + k2 + seed)
    n1, n2 = k1 + extra1, k2 + extra2
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    a1 = rng.uniform(0, 360, n1).astype(f32)
    h1 = np.zeros(n1, np.uint8)
    h1[rng.permutation(n1)[:k1]] = 1
    d2, a2 = _neighbour_descriptors(rng, d1, a1, np.arange(n1), n2)
    h2 = np.zeros(n2, np.uint8)
    h2[rng.permutation(n2)[:k2]] = 1
    return dict(kf1=keyframe(one_node(rng.permutation(n1)), d1, a1, h1), neighbours=[keyframe(one_node(rng.permutation(n2)), d2, a2, h2)])


# ---- hand-built cases ---------------------------------------------------------------------------------------------------------
def bits(*ranges):
    """a descriptor with the bits of the given (first, end) ranges set: the distance of two such descriptors is the size of the
    symmetric difference of their bit sets"""
    b = np.zeros(256, np.uint8)
    for lo, hi in ranges:
        b[lo:hi] = 1
    return np.packbits(b)


Z = bits()


def _fv(lists):
    """lists: {node: [features in list order]} -> CSR"""
    nodes = sorted(lists)
    off = np.cumsum([0] + [len(lists[n]) for n in nodes]).astype(np.int32)
    feats = np.array([f for n in nodes for f in lists[n]], np.uint32)
    return dict(fv_nodes=np.array(nodes, np.uint32), fv_offsets=off, fv_features=feats)


def _hand_kf(desc, lists, angles=None, has_point=None, n_left=-1, n_un=None):
    n = len(desc)
    return keyframe(_fv(lists), np.array(desc, np.uint8).reshape(n, 32), np.zeros(n) if angles is None else angles,
                    np.ones(n, np.uint8) if has_point is None else has_point, n_left, n_un)


def angles_decide(ang1, ang2, seed=7):
    """Two sides whose angles alone decide: feature i of side 1 (angle ang1[i]) has a vocabulary node of its own, and so has feature
    i of side 2 (angle ang2[i]), a copy of it - one candidate at distance 0 each, so every feature i < len(ang2) matches feature i
    before the rotation filter and the others nothing.  -> (descriptors [n1, 32], lists of side 1, lists of side 2); side 2 takes
    the first len(ang2) descriptors"""
    n1, n2 = len(ang1), len(ang2)
    assert n2 <= n1
    d = np.random.default_rng(seed).integers(0, 256, (n1, 32), dtype=np.uint8)
    return d, {10 + i: [i] for i in range(n1)}, {10 + i: [i] for i in range(n2)}


def rotation_table():
    """ROTATION_CASES of tests/test_search_geometry_cpu.py - bin -> count with the bins that survive ComputeThreeMaxima listed by
    hand - without `doubles` (two writes to one keypoint: specific to the last-frame search) -> [(name, rot [n] float32 degrees,
    kept [n] bool, number kept)]: one match per count of a bin with rotation 30 * bin, in the order of the spec.  The bin of a
    rotation is written as in rotation_expectation there; no library code takes part."""
    from tests.test_search_geometry_cpu import ROTATION_CASES
    out = []
    for name, (spec, _, kept_bins, n_kept) in ROTATION_CASES.items():
        if name == "doubles":
            continue
        rot = np.array([30.0 * b for b, cnt in spec.items() for _ in range(cnt)], f32)
        bins = np.round(np.mod(rot.astype(np.float64), 360.0) / 30.0).astype(int)
        kept = np.isin(bins, sorted(kept_bins))
        assert len(rot) <= 200 and int(kept.sum()) == n_kept, name
        out.append((name, rot, kept, n_kept))
    return out


def rotation_cases():
    """the table above as cases of hand_built()'s form: one per histogram, check_orientation on, and `rotation_all_in_one_call`
    (on and off) with every histogram as a neighbour of the SAME keyframe 1 - angle 0 everywhere, so a match's rotation is minus
    the neighbour's angle.  A neighbour has as many features as its histogram has matches."""
    table = rotation_table()
    out = []

    def case(name, n1, rots, ori):
        d, lists1, _ = angles_decide(np.zeros(n1), [])
        nbs, want = [], np.full((len(rots), n1), -1, np.int32)
        for k, (rot, kept) in enumerate(rots):
            nbs.append(_hand_kf(d[:len(rot)], {10 + i: [i] for i in range(len(rot))}, angles=-rot))
            hit = np.nonzero(kept | (not ori))[0]
            want[k, hit] = hit
        out.append(dict(name=name, kf1=_hand_kf(d, lists1, angles=np.zeros(n1)), neighbours=nbs, nn_ratio=0.9, check_orientation=ori,
                        matches12=want, n=(want >= 0).sum(axis=1).astype(np.int32)))

    for name, rot, kept, _ in table:
        case("rotation_" + name, max(len(rot), 1), [(rot, kept)], True)
    n1 = max(len(rot) for _, rot, _, _ in table)
    for ori in (True, False):
        case("rotation_all_in_one_call" + ("" if ori else "_filter_off"), n1, [(rot, kept) for _, rot, kept, _ in table], ori)
    return out


def hand_built():
    """-> list of dict(name, kf1, neighbours, nn_ratio, check_orientation, matches12 [J, n1], n [J]): the expected outputs are
    written out from the reference text, not computed"""
    out = []

    def case(name, kf1, neighbours, nn_ratio, ori, matches12, n):
        out.append(dict(name=name, kf1=kf1, neighbours=list(neighbours), nn_ratio=nn_ratio, check_orientation=ori,
                        matches12=np.asarray(matches12, np.int32).reshape(len(neighbours), -1), n=np.asarray(n, np.int32)))

    # bestDist1 < TH_LOW is strict (:947): 49 matches, 50 does not (two nodes, one candidate each)
    case("th_low_49_and_50", _hand_kf([Z, Z], {5: [0], 9: [1]}), [_hand_kf([bits((0, 49)), bits((0, 50))], {5: [0], 9: [1]})],
         0.9, False, [[0, -1]], [1])
    # one candidate: bestDist2 stays 256.  40 < 0.15664f * 256 = 40.0998, but not < 0.15664f * 255 = 39.94
    case("single_candidate_second_is_256", _hand_kf([Z], {5: [0]}), [_hand_kf([bits((0, 40))], {5: [0]})], 0.15664, False, [[0]], [1])
    case("single_candidate_ratio_fails", _hand_kf([Z], {5: [0]}), [_hand_kf([bits((0, 40))], {5: [0]})], 0.15, False, [[-1]], [0])
    # two candidates at the best distance (10): bestDist2 == bestDist1, the ratio fails at nn_ratio <= 1 and nothing is claimed ...
    tie = _hand_kf([bits((0, 10)), bits((10, 20))], {5: [1, 0]})
    case("tie_fails_the_ratio_at_1", _hand_kf([Z], {5: [0]}), [tie], 1.0, False, [[-1]], [0])
    case("tie_fails_the_ratio_at_0_9", _hand_kf([Z], {5: [0]}), [tie], 0.9, False, [[-1]], [0])
    # ... and at 1.5 the first of the list wins (the list is 1, 0)
    case("tie_first_of_the_list_wins", _hand_kf([Z], {5: [0]}), [tie], 1.5, False, [[1]], [1])
    # two keyframe-1 features share their nearest candidate c0 (3 and 5 bits away); c1 is 20 / 22 away, c2 30 / 32.  The first in
    # list order takes c0, the second then takes c1 with the ratio formed over c1, c2: 22 < 0.9 * 32
    two1 = [Z, bits((200, 202))]
    cands = [bits((0, 3)), bits((0, 20)), bits((0, 30))]
    case("shared_nearest_first_in_list_order", _hand_kf(two1, {5: [0, 1]}), [_hand_kf(cands, {5: [0, 1, 2]})], 0.9, False, [[0, 1]], [2])
    case("shared_nearest_list_order_reversed", _hand_kf(two1, {5: [1, 0]}), [_hand_kf(cands, {5: [0, 1, 2]})], 0.9, False, [[1, 0]], [2])
    # with c2 at 22 / 24 instead the second feature's ratio over what is left fails: 22 < 0.9 * 24 = 21.6 is false
    case("shared_nearest_second_fails_over_what_is_left", _hand_kf(two1, {5: [0, 1]}),
         [_hand_kf([bits((0, 3)), bits((0, 20)), bits((0, 22))], {5: [0, 1, 2]})], 0.9, False, [[0, -1]], [1])
    # the list of keyframe 2 in descending index order: features 2 and 0 are both 8 bits away, list order decides, not index order
    case("descending_list_order", _hand_kf([Z], {5: [0]}), [_hand_kf([bits((0, 8)), bits((0, 30)), bits((8, 16))], {5: [2, 1, 0]})],
         1.5, False, [[2]], [1])
    # a candidate without a point is neither best (c0, 2 bits away) nor second best (c2, 11 away: 10 < 0.9 * 11 would fail)
    case("candidate_without_point", _hand_kf([Z], {5: [0]}),
         [_hand_kf([bits((0, 2)), bits((0, 10)), bits((0, 11))], {5: [0, 1, 2]}, has_point=[0, 1, 0])], 0.9, False, [[1]], [1])
    # a keyframe-1 feature without a point is skipped
    case("feature_without_point", _hand_kf([Z, Z], {5: [0, 1]}, has_point=[0, 1]), [_hand_kf([bits((0, 2))], {5: [0]})], 0.9, False,
         [[-1, 0]], [1])
    # two cameras: idx >= n_un is skipped on either side even with has_point set.  Keyframe 1: features 2, 3 are right-camera ones;
    # keyframe 2: only c0 (5 bits from feature 0) is a left one, c1 (a copy of feature 0) and c2 (a copy of feature 2) are not
    A, B, Cc = bits((100, 140)), bits((150, 200)), bits((200, 256))
    k1d, k2d = [Z, A, B, Cc], [bits((0, 5)), Z, B]
    case("two_cameras_skip_beyond_n_un", _hand_kf(k1d, {5: [0, 1, 2, 3]}, n_left=2, n_un=2), [_hand_kf(k2d, {5: [0, 1, 2]}, n_left=1, n_un=1)],
         0.9, False, [[0, -1, -1, -1]], [1])
    # n_left == -1 ignores n_un: feature 0 takes its copy c1 (0 < 0.9 * 5), feature 1 takes c0 (45 < 0.9 * 90), feature 2 its copy c2,
    # feature 3 finds nothing left
    case("one_camera_ignores_n_un", _hand_kf(k1d, {5: [0, 1, 2, 3]}, n_left=-1, n_un=2), [_hand_kf(k2d, {5: [0, 1, 2]}, n_left=-1, n_un=1)],
         0.9, False, [[1, 0, 2, -1]], [3])
    # the histogram: feature i has its own node and one candidate at distance 0, so everything matches and the angles decide.
    # bin = round(rot / 30) with rot = angle1 - angle2 (+ 360 when negative): ten features with rot = 10 - 350 < 0 -> 20 -> bin 1;
    # three with rot = 900 -> bin 30 -> 0 and three with rot = 5 -> bin 0; five in bin 5, four in bin 8, one in bin 10.
    # Bins 1, 0 and 5 are kept (10, 6, 5).
    groups = [(10, 10.0, 350.0, True), (3, 900.0, 0.0, True), (3, 5.0, 0.0, True), (5, 150.0, 0.0, True), (4, 240.0, 0.0, False),
              (1, 300.0, 0.0, False)]

    def histogram_case(name, groups, ori=True):
        ang1 = [a for cnt, a, _, _ in groups for _ in range(cnt)]
        ang2 = [b for cnt, _, b, _ in groups for _ in range(cnt)]
        kept = [k for cnt, _, _, k in groups for _ in range(cnt)]
        n = len(ang1)
        d, lists, _ = angles_decide(ang1, ang2)
        want = [i if (kept[i] or not ori) else -1 for i in range(n)]
        case(name, _hand_kf(d, lists, angles=ang1), [_hand_kf(d, lists, angles=ang2)], 0.9, ori, [want], [sum(w >= 0 for w in want)])

    histogram_case("histogram_negative_rot_and_wrap", groups)
    histogram_case("histogram_off_keeps_everything", groups, ori=False)
    # the 10 % rule: max2 = 2 < 0.1 * 21 drops the second and the third maximum; max2 = 3, max3 = 2 drops the third only
    histogram_case("histogram_10_percent_drops_second_and_third", [(21, 40.0, 0.0, True), (2, 100.0, 0.0, False), (1, 200.0, 0.0, False)])
    histogram_case("histogram_10_percent_drops_third", [(21, 40.0, 0.0, True), (3, 100.0, 0.0, True), (2, 200.0, 0.0, False)])
    # a node present on one side only: node 3's feature has its copy under node 9 of keyframe 2 and stays unmatched
    case("node_on_one_side_only", _hand_kf([Z, A], {3: [0], 7: [1]}), [_hand_kf([Z, A], {9: [0], 7: [1]})], 0.9, False, [[-1, 1]], [1])
    case("no_shared_node", _hand_kf([Z, A], {3: [0], 7: [1]}), [_hand_kf([Z, A], {4: [0], 9: [1]})], 0.9, False, [[-1, -1]], [0])
    # the same keyframe-2 index matched in two neighbours of one call: claims do not travel between neighbours
    nb = _hand_kf(cands, {5: [0, 1, 2]})
    case("same_index_in_two_neighbours", _hand_kf(two1, {5: [0, 1]}), [nb, nb], 0.9, False, [[0, 1], [0, 1]], [2, 2])
    return out


def to_device(orb, kf):
    """a keyframe dict as the library's BowKeyFrame"""
    side = orb.BowSide(kf["fv_nodes"], kf["fv_offsets"], kf["fv_features"], kf["descriptors"], kf["angles"])
    return orb.BowKeyFrame(side, kf["has_point"], kf["n_left"], kf["n_un"])

"""Inputs of ORBmatcher::SearchByBoW(KeyFrame, Frame) as Tracking::Relocalization calls it - one frame against N candidate
keyframes - for the tests of ft_search_by_bow_candidates: seeded scenarios, single-node cases of a given size, and hand-built
cases whose expected outputs are written out from the reference text (src/ORBmatcher.cc:322-524).  A side is a dict with
fv_nodes, fv_offsets, fv_features, descriptors, angles (what oracle.binding.search_by_bow takes); a candidate also has has_point.
oracle() runs the oracle per candidate, to_device() builds the library's records.
"""
import functools

import numpy as np

from oracle import binding as ob
from tests import bow_kf_cases as bk

f32 = np.float32
vocabulary = bk.vocabulary
bits = bk.bits
Z = bits()


def side(fv, descriptors, angles, has_point=None):
    d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
    s = dict(fv_nodes=np.asarray(fv["fv_nodes"], np.uint32), fv_offsets=np.asarray(fv["fv_offsets"], np.int32),
             fv_features=np.asarray(fv["fv_features"], np.uint32), descriptors=d, angles=np.asarray(angles, f32))
    if has_point is not None:
        s["has_point"] = np.asarray(has_point, np.uint8)
    return s


EMPTY_FV = dict(fv_nodes=[], fv_offsets=[0], fv_features=[])


def _candidate_arrays(rng, dF, aF, pool, n):
    """n descriptors and angles of a candidate drawn from the frame's (dF, aF): 70 % copies with 0 - 14 flipped bits, 15 % with
    40 - 60 (around TH_LOW), 15 % random; the angles are the frame's plus one rotation, sigma = 4 degrees, 20 % uniform outliers"""
    src = pool[rng.integers(0, len(pool), n)]
    kind = rng.random(n)
    d = np.zeros((n, 32), np.uint8)
    close, mid, rnd = kind < 0.7, (kind >= 0.7) & (kind < 0.85), kind >= 0.85
    d[close] = bk._near(rng, dF[src[close]], 0, 14)
    d[mid] = bk._near(rng, dF[src[mid]], 40, 60)
    d[rnd] = rng.integers(0, 256, (int(rnd.sum()), 32), dtype=np.uint8)
    rot = f32(rng.uniform(0, 360))
    a = (aF[src] + rot + rng.normal(0, 4, n)).astype(f32)
    outl = rng.random(n) < 0.2
    a[outl] = rng.uniform(0, 360, int(outl.sum()))
    return d, np.mod(a, f32(360)).astype(f32)


@functools.lru_cache(maxsize=None)
def scenario(seed, n_f=600, n_k=(500, 64, 700, 300), levelsup=2, two_cam=False, empty_candidate=False, pointless_candidate=False,
             foreign_candidate=False, vocab=(10, 4, 17), has=0.8):
    """a frame of n_f features against len(n_k) candidates -> dict(frame, nleft, candidates).  empty_candidate /
    pointless_candidate / foreign_candidate: one more candidate with no feature / without a map point / with features of other
    vocabulary nodes only."""
    rng = np.random.default_rng(seed)
    voc, ovoc = vocabulary(*vocab)
    centres = voc["descriptors"][1:]
    dF = bk._near(rng, centres[rng.integers(0, len(centres), n_f)], 0, 20)
    dup = rng.random(n_f) < 0.1  # exact copies of another descriptor of the frame: ties in scan order
    dF[dup] = dF[rng.integers(0, n_f, int(dup.sum()))]
    aF = rng.uniform(0, 360, n_f).astype(f32)
    frame = side(ovoc.transform(dF, levelsup), dF, aF)
    cands = []
    for m in n_k:
        d, a = _candidate_arrays(rng, dF, aF, np.arange(n_f), m)
        cands.append(side(ovoc.transform(d, levelsup), d, a, rng.random(m) < has))
    if empty_candidate:
        cands.insert(1, side(EMPTY_FV, np.zeros((0, 32), np.uint8), [], []))
    if pointless_candidate:
        cands.insert(3, dict(cands[0], has_point=np.zeros_like(cands[0]["has_point"])))
    if foreign_candidate:
        cands.append(dict(cands[0], fv_nodes=(cands[0]["fv_nodes"] + np.uint32(100000)).astype(np.uint32)))
    return dict(frame=frame, nleft=int(0.55 * n_f) if two_cam else -1, candidates=cands)


# The scenarios the CPU and the GPU tests share, (seed, keyword arguments): ~100 nodes with one and two cameras, 10 nodes, and one
# node of nearly all the frame's 700 features (the path of the frame nodes too long for the registers).
MAIN = [(61, dict(levelsup=2)), (62, dict(levelsup=2, n_f=700, two_cam=True)), (63, dict(levelsup=3)),
        (64, dict(levelsup=4, n_f=700, n_k=(700, 650)))]
CONFIGS = [(0.75, True), (0.9, True), (0.6, False)]  # (nn_ratio, check_orientation)


def main_scenario(i):
    seed, kw = MAIN[i]
    return scenario(seed, **kw)


def one_node(order, node=0):
    return bk.one_node(order, node)


@functools.lru_cache(maxsize=None)
def node_size_case(k_kf, k_f, two_cam=False, seed=0):
    """ONE shared node, written directly: k_f random frame descriptors, k_kf candidate descriptors that are copies with 0 - 30
    flipped bits, every one with a point; both lists in shuffled order"""
    rng = np.random.default_rng(100000 * k_kf + 10 * k_f + int(two_cam) + 7919 * seed)
    dF = rng.integers(0, 256, (k_f, 32), dtype=np.uint8)
    aF = rng.uniform(0, 360, k_f).astype(f32)
    src = rng.integers(0, k_f, k_kf)
    dK = bk._near(rng, dF[src], 0, 30)
    aK = np.mod(aF[src] + f32(rng.uniform(0, 360)) + rng.normal(0, 4, k_kf), 360).astype(f32)
    frame = side(one_node(rng.permutation(k_f)), dF, aF)
    cand = side(one_node(rng.permutation(k_kf)), dK, aK, np.ones(k_kf, np.uint8))
    return dict(frame=frame, nleft=int(0.55 * k_f) if two_cam else -1, candidates=[cand])


@functools.lru_cache(maxsize=None)
def many_small(n_candidates=70, n=64, seed=71):
    """n_candidates candidates of n features against a frame of 300 (levelsup 3)"""
    return scenario(seed, n_f=300, n_k=(n,) * n_candidates, levelsup=3)


def oracle(S, nn_ratio=0.75, ori=True, candidates=None):
    """the oracle's SearchByBoW(KeyFrame, Frame), one call per candidate -> list of dict(matches, n)"""
    cs = S["candidates"] if candidates is None else candidates
    return [ob.search_by_bow(c, c["has_point"], S["frame"], S["nleft"], nn_ratio, ori) for c in cs]


@functools.lru_cache(maxsize=None)
def oracle_main(i, cfg):
    return oracle(main_scenario(i), *cfg)


# ---- hand-built cases ---------------------------------------------------------------------------------------------------------
def _hand_side(desc, lists, has_point=False):
    n = len(desc)
    return side(bk._fv(lists), np.array(desc, np.uint8).reshape(n, 32), np.zeros(n), np.ones(n, np.uint8) if has_point else None)


def hand_built():
    """-> list of dict(name, frame, nleft, candidates, nn_ratio, check_orientation, matches [N, n_f], n [N]): the expected outputs
    are written out from the reference text, not computed.  bits((a, b)) sets bits a .. b - 1, so the distance of two such
    descriptors is the size of the symmetric difference."""
    out = []

    def case(name, kf_desc, kf_lists, f_desc, f_lists, nleft, nn_ratio, matches, n):
        out.append(dict(name=name, frame=_hand_side(f_desc, f_lists), nleft=nleft, candidates=[_hand_side(kf_desc, kf_lists, True)],
                        nn_ratio=nn_ratio, check_orientation=False, matches=np.asarray(matches, np.int32).reshape(1, -1),
                        n=np.asarray(n, np.int32)))

    # bestDist1 <= TH_LOW (:426): 50 matches, 51 does not (two nodes, one frame feature each: bestDist2 stays 256)
    case("th_low_50_and_51", [Z, Z], {5: [0], 9: [1]}, [bits((0, 50)), bits((0, 51))], {5: [0], 9: [1]}, -1, 0.75, [0, -1], [1])
    # the frame's list is 2, 1, 0; features 2 and 0 are both 8 bits away: the first of the list wins (1.5: 8 < 1.5 * 8)
    case("tie_first_in_list_order", [Z], {5: [0]}, [bits((0, 8)), bits((0, 30)), bits((8, 16))], {5: [2, 1, 0]}, -1, 1.5, [-1, -1, 0], [1])
    # ... and at 0.9 the tie fails the ratio
    case("tie_fails_the_ratio", [Z], {5: [0]}, [bits((0, 8)), bits((0, 30)), bits((8, 16))], {5: [2, 1, 0]}, -1, 0.9, [-1, -1, -1], [0])
    # two keyframe features share their nearest frame feature f0 (3 and 5 bits away); f1 is 20 / 22 away, f2 30 / 32.  The first in
    # list order takes f0, the second skips it and takes f1 with the ratio formed over f1, f2: 22 < 0.9 * 32
    two = [Z, bits((200, 202))]
    three = [bits((0, 3)), bits((0, 20)), bits((0, 30))]
    case("claimed_feature_passes_to_second_choice", two, {5: [0, 1]}, three, {5: [0, 1, 2]}, -1, 0.9, [0, 1, -1], [2])
    case("claimed_feature_list_order_reversed", two, {5: [1, 0]}, three, {5: [0, 1, 2]}, -1, 0.9, [1, 0, -1], [2])
    # two cameras, Nleft = 2: left f0 (5), f1 (40) - 5 < 0.75 * 40; right f2 (10), f3 (11) - 10 < 0.75 * 11 fails, and is kept (:458)
    case("right_match_with_failing_ratio_is_kept", [Z], {5: [0]}, [bits((0, 5)), bits((0, 40)), bits((0, 10)), bits((0, 11))],
         {5: [0, 1, 2, 3]}, 2, 0.75, [0, -1, 0, -1], [2])
    # the left best is 51: the right camera (5 bits away) is not looked at (:426 encloses :456)
    case("right_match_suppressed_by_left_51", [Z], {5: [0]}, [bits((0, 51)), bits((0, 5))], {5: [0, 1]}, 1, 0.75, [-1, -1], [0])
    # the left best is 10 <= 50 but 10 < 0.75 * 11 fails: no left match, the right one (5) is made all the same
    case("right_match_kept_when_left_ratio_fails", [Z], {5: [0]}, [bits((0, 10)), bits((0, 11)), bits((0, 5))], {5: [0, 1, 2]}, 2, 0.75,
         [-1, -1, 0], [1])
    return out


def rotation_cases():
    """the directed histograms of the rotation filter (bow_kf_cases.rotation_table) as cases of hand_built()'s form: one per
    histogram, and `rotation_all_in_one_call` (filter on and off) with every histogram as a candidate of the SAME frame.  The bin is
    the keyframe's angle minus the frame's (:491) while the row is the frame's: the frame's angles are 0 and a candidate's are
    its matches' rotations - the other way round than for the keyframe matcher."""
    table = bk.rotation_table()
    out = []

    def case(name, n_f, rots, ori):
        d, lists, _ = bk.angles_decide(np.zeros(n_f), [])
        cands, want = [], np.full((len(rots), n_f), -1, np.int32)
        for k, (rot, kept) in enumerate(rots):
            n = len(rot)
            cands.append(side(bk._fv({10 + i: [i] for i in range(n)}), d[:n], rot, np.ones(n, np.uint8)))
            hit = np.nonzero(kept | (not ori))[0]
            want[k, hit] = hit
        out.append(dict(name=name, frame=side(bk._fv(lists), d, np.zeros(n_f)), nleft=-1, candidates=cands, nn_ratio=0.75,
                        check_orientation=ori, matches=want, n=(want >= 0).sum(axis=1).astype(np.int32)))

    for name, rot, kept, _ in table:
        case("rotation_" + name, max(len(rot), 1), [(rot, kept)], True)
    n_f = max(len(rot) for _, rot, _, _ in table)
    for ori in (True, False):
        case("rotation_all_in_one_call" + ("" if ori else "_filter_off"), n_f, [(rot, kept) for _, rot, kept, _ in table], ori)
    return out


def to_device(orb, S, candidates=None):
    """-> (BowSide of the frame, [BowCandidate])"""
    f = S["frame"]
    cs = S["candidates"] if candidates is None else candidates
    mk = lambda s: orb.BowSide(s["fv_nodes"], s["fv_offsets"], s["fv_features"], s["descriptors"], s["angles"])
    return mk(f), [orb.BowCandidate(mk(c), c["has_point"]) for c in cs]

"""The restatement of the KeyFrameDatabase queries (tests/kfdb_ref.py) pinned on independent formulations and hand-computed
cases: it is what ft_kfdb_* is compared with on the device, so it is checked here without one."""
import numpy as np
import pytest

from tests import kfdb_cases as kc
from tests import kfdb_ref as kr

PLACE, RELOC = kc.PLACE, kc.RELOC


def _vec(ids, values=None):
    ids = np.array(ids, np.uint32)
    v = np.ones(len(ids)) if values is None else np.array(values, np.float64)
    return ids, v / v.sum()


def test_counts_are_set_intersections():
    rng = np.random.default_rng(1)
    for trial in range(30):
        db = kr.KeyFrameDatabase()
        vecs = [kc.make_vector(rng, 256, int(rng.integers(0, 120))) for _ in range(40)]
        for v in vecs:
            db.add(*v)
        q = kc.make_vector(rng, 256, int(rng.integers(1, 120)))
        for kind in (PLACE, RELOC):
            r = db.score(kind, trial + 1, *q)
            common = [len(set(v[0].tolist()) & set(q[0].tolist())) for v in vecs]
            _, words, _ = db.state(kind, range(40))
            assert words.tolist() == common
            assert r["n_sharing"] == sum(c > 0 for c in common) and r["max_common_words"] == max(common)
            assert r["handles"].tolist() == [h for h in r["listed"] if common[h] > r["min_common_words"]]


def test_score_is_one_minus_half_the_l1_distance():
    rng = np.random.default_rng(2)
    for _ in range(200):
        W = 64
        a, b = kc.make_vector(rng, W, int(rng.integers(1, W))), kc.make_vector(rng, W, int(rng.integers(1, W)))
        da, db_ = np.zeros(W), np.zeros(W)
        da[a[0]], db_[b[0]] = a[1], b[1]
        raw, si = kr.l1_score(a[0].tolist(), list(a[1]), b[0].tolist(), list(b[1]))
        assert abs(raw - (1.0 - 0.5 * np.abs(da - db_).sum())) < 1e-12   # a bound on the restatement, not on the device
        assert si == np.float32(raw) and isinstance(raw, np.float64)


def test_list_order_is_first_shared_word_then_add_sequence():
    rng = np.random.default_rng(3)
    for trial in range(200):
        db = kr.KeyFrameDatabase()
        W = int(rng.choice([16, 64, 256]))
        vecs = {}
        for _ in range(int(rng.integers(1, 30))):
            v = kc.make_vector(rng, W, int(rng.integers(0, W // 2)))
            vecs[db.add(*v)] = v
        for h in [h for h in list(vecs) if rng.random() < 0.3]:
            db.erase(h)
            del vecs[h]
        for _ in range(int(rng.integers(0, 10))):
            v = kc.make_vector(rng, W, int(rng.integers(0, W // 2)))
            vecs[db.add(*v)] = v
        q = kc.make_vector(rng, W, int(rng.integers(1, W // 2)))
        connected = [h for h in vecs if rng.random() < 0.2]
        r = db.score(PLACE, 1, *q, connected)
        keys = []
        for h, v in vecs.items():
            shared = sorted(set(v[0].tolist()) & set(q[0].tolist()))
            if shared and h not in connected:
                keys.append((shared[0], h))
        assert r["listed"] == [h for _, h in sorted(keys)], trial


@pytest.mark.parametrize("max_words,threshold,scored", [(5, 4, [5]), (10, 8, [9, 10]), (15, 12, [13, 14, 15])])
def test_threshold_is_one_float_product_truncated_and_strict(max_words, threshold, scored):
    exp = kc.expected("threshold_%d" % max_words)
    for e in (x for x in exp if isinstance(x, dict)):
        r = e["result"]
        assert (r["max_common_words"], r["min_common_words"]) == (max_words, threshold)
        assert r["words"].tolist() == scored          # a keyframe with exactly `threshold` words is rejected
        assert r["n_sharing"] == max_words


def test_connected_keyframes_end_with_count_one_and_keep_their_stamp():
    db = kr.KeyFrameDatabase()
    a = db.add(*_vec([1, 2, 3, 4]))
    b = db.add(*_vec([2, 3, 4, 9]))
    r = db.score(PLACE, 7, *_vec([1, 2, 3, 4]), connected=[b])
    assert r["listed"] == [a] and r["handles"].tolist() == [a]
    stamps, words, _ = db.state(PLACE, [a, b])
    assert stamps.tolist() == [7, 0] and words.tolist() == [4, 1]
    # the relocalisation query knows no connected set and has its own members
    r = db.score(RELOC, 7, *_vec([1, 2, 3, 4]))
    assert r["listed"] == [a, b] and db.state(RELOC, [a, b])[1].tolist() == [4, 3]


def test_stale_score_of_a_neighbour_is_added():
    """:689: a neighbour that shares a word in this query (so it carries the stamp) but is below the threshold adds the score an
    EARLIER query left in it"""
    db = kr.KeyFrameDatabase()
    a = db.add(*_vec(range(0, 10)))
    b = db.add(*_vec([0, 20, 21, 22]))
    r1 = db.score(PLACE, 1, *_vec([0, 20, 21, 22]))          # scores b (4 words) only: a shares 1 of max 4
    assert r1["handles"].tolist() == [b]
    stale = db.state(PLACE, [b])[2][0]
    assert stale == np.float32(1.0)
    r2 = db.score(PLACE, 2, *_vec(range(0, 10)))             # lists both, scores a only
    assert r2["listed"] == [a, b] and r2["handles"].tolist() == [a]
    assert db.state(PLACE, [b])[0][0] == 2 and db.state(PLACE, [b])[2][0] == stale
    loop, merge = db.select_n_best(2, r2, lambda h: [b], lambda h: 0, 0, 3)
    acc, _ = db._accumulate(PLACE, 2, r2, lambda h: [b])
    assert acc[0][0] == np.float32(r2["scores"][0] + stale) and acc[0][1] == a   # 1.0 does not exceed a's own 1.0: strict >
    assert loop == [a] and merge == []


def test_equal_accumulated_scores_keep_list_order():
    entries = [(np.float32(0.5), 10), (np.float32(0.75), 11), (np.float32(0.5), 12), (np.float32(0.75), 13), (np.float32(0.5), 14)]
    assert [h for _, h in kr._list_sort_descending(entries)] == [11, 13, 10, 12, 14]
    db = kr.KeyFrameDatabase()
    hs = [db.add(*_vec([1, 2, 3])) for _ in range(4)]
    r = db.score(PLACE, 1, *_vec([1, 2, 3]))
    assert r["handles"].tolist() == hs and len(set(r["scores"].tolist())) == 1
    loop, merge = db.select_n_best(1, r, lambda h: [], lambda h: h % 2, 0, 1)
    assert loop == [hs[0]] and merge == [hs[1]]


def test_repeated_query_id_lists_nobody_again_and_accumulates():
    db = kr.KeyFrameDatabase()
    a = db.add(*_vec([1, 2, 3]))
    r1 = db.score(PLACE, 4, *_vec([1, 2, 3]))
    r2 = db.score(PLACE, 4, *_vec([2, 3]))
    assert r1["n_sharing"] == 1 and r2["n_sharing"] == 0 and len(r2["handles"]) == 0
    assert db.state(PLACE, [a])[1].tolist() == [5]
    fresh = db.add(*_vec([1, 2, 3]))
    assert db.score(PLACE, 0, *_vec([1, 2, 3]))["listed"] == [a]       # a fresh keyframe is stamped 0 already
    assert db.state(PLACE, [fresh])[1].tolist() == [3]


def test_relocalisation_keeps_strictly_more_than_three_quarters():
    db = kr.KeyFrameDatabase()
    hs = [db.add(*_vec([1])) for _ in range(3)]
    scored = dict(handles=np.array(hs, np.int32), scores=np.array([1.0, 0.75, 0.7500001], np.float32))
    assert db.select_reloc(9, scored, lambda h: [], lambda h: 0, 0) == [hs[0], hs[2]]
    assert db.select_reloc(9, scored, lambda h: [], lambda h: 1 if h == hs[0] else 0, 0) == [hs[2]]


def test_summation_order_shows_in_the_doubles_and_not_in_the_floats():
    """The power of comparing raw_scores: adding the same terms in descending word order changes at least half of the scored
    keyframes' doubles, and none of their floats - the float output alone could not tell the orders apart."""
    doubles = floats = total = 0
    for name in kc.ORDER_NAMES:
        ops, exp = kc.ops(name), kc.expected(name)
        vectors = ops[0][1]
        _, _, _, q_ids, q_vals, _ = ops[1]
        r = exp[1]["result"]
        assert len(r["handles"]) >= 30 and 16 <= r["words"].min() and r["words"].max() <= 110
        print(name, "common words %d - %d" % (r["words"].min(), r["words"].max()))
        for h, raw, si in zip(r["handles"], r["raw_scores"], r["scores"]):
            ids, vals = vectors[int(h)]
            fwd = kr.l1_score(q_ids.tolist(), list(q_vals), ids.tolist(), list(vals))
            rev = kr.l1_score(q_ids.tolist(), list(q_vals), ids.tolist(), list(vals), reverse=True)
            assert fwd[0] == raw and fwd[1] == si
            doubles += fwd[0] != rev[0]
            floats += fwd[1] != rev[1]
            total += 1
    print("order cases: %d scored, %d doubles and %d floats differ under the reversed sum" % (total, doubles, floats))
    assert 2 * doubles >= total, (doubles, total)
    assert floats == 0

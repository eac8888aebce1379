"""ft_kfdb_* on the device against the sequential restatement of the reference's KeyFrameDatabase (tests/kfdb_ref.py): every output
of every query, the state of both kinds in every live keyframe after each query, and the doubles before the rounding to float,
bit for bit - no tolerance and no excluded case.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from fasttrack_amd import _capi, orb, synth
from tests import kfdb_cases as kc
from tests import kfdb_ref as kr

pytestmark = pytest.mark.gpu

PLACE, RELOC = kc.PLACE, kc.RELOC


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_result(got, want, where):
    for key in ("n_sharing", "max_common_words", "min_common_words"):
        assert got[key] == want[key], (where, key, got[key], want[key])
    for key in ("handles", "words", "scores", "raw_scores"):
        assert got[key].dtype == want[key].dtype and np.array_equal(_bits(got[key]), _bits(want[key])), (where, key, got[key][:8], want[key][:8])


def _same_state(db, e, where):
    for kind in (PLACE, RELOC):
        got, want = db.state(kind, e["live"]), e["state"][kind]
        for g, w, what in zip(got, want, ("stamp", "words", "score")):
            assert np.array_equal(_bits(g), _bits(w)), (where, kind, what, np.nonzero(_bits(g) != _bits(w))[0][:8])
    assert db.size()[0] == len(e["live"])


def _replay(ctx, name, after_query=None):
    db = orb.KeyFrameDatabase(ctx)
    try:
        for k, (op, e) in enumerate(zip(kc.ops(name), kc.expected(name))):
            got = kc.replay(db, op)
            if op[0] == "add":
                assert got == e, (name, k)
            elif op[0] == "query":
                _same_result(got, e["result"], (name, k))
                _same_state(db, e, (name, k))
                if after_query:
                    after_query(db, k, op, got, e)
    finally:
        db.close()


@pytest.mark.parametrize("name", kc.NAMES)
def test_cases_match_the_restatement(ctx, name):
    _replay(ctx, name)


def test_compaction_happens_and_keeps_handles(ctx):
    ctx.reset_stats()
    _replay(ctx, "compaction")
    assert ctx.get_stat("kfdb.compactions")[1] >= 1
    ctx.reset_stats()
    _replay(ctx, "three_queries")                      # nothing erased: nothing compacted
    assert ctx.get_stat("kfdb.compactions") == (0.0, 0)


def test_a_query_is_two_launches_whatever_the_database(ctx):
    try:
        ctx.set_kernel_timing(True)
        counts = []
        for name in ("db_1", "db_65", "db_300"):
            ctx.reset_stats()
            _replay(ctx, name)
            total, calls = ctx.get_stat("kfdb_score.launches")
            assert total == 2 * calls and calls >= 1, (name, total, calls)
            assert ctx.get_stat("kernel.kfdb_count")[1] == calls == ctx.get_stat("kernel.kfdb_score")[1]
            counts.append(calls)
        ctx.reset_stats()
        _replay(ctx, "db_0")                            # an empty database: no launch
        db = orb.KeyFrameDatabase(ctx)
        db.add([kc.make_vector(np.random.default_rng(0), 64, 10), (np.zeros(0, np.uint32), np.zeros(0))])
        r = db.score(PLACE, 1, np.zeros(0, np.uint32), np.zeros(0))    # an empty query
        assert (r["n_sharing"], r["max_common_words"], r["min_common_words"], len(r["handles"])) == (0, 0, 0, 0)
        db.erase([0])
        r = db.score(PLACE, 1, *kc.make_vector(np.random.default_rng(0), 64, 10))   # the live keyframe holds no word
        assert r["n_sharing"] == 0 and db.size() == (1, 0)
        db.close()
        assert ctx.get_stat("kfdb_score.launches") == (0.0, 0) == ctx.get_stat("kernel.kfdb_count")
    finally:
        ctx.set_kernel_timing(False)


# ---- the selection calls, on the state the queries of a case left ----
def _neighbours_of(live, seed, mode):
    live = list(live)

    def neighbours(h):
        rng = np.random.default_rng([seed, h])
        if mode == "none" or not live:
            return []
        n = int(rng.integers(0, 11))
        return [int(x) for x in rng.choice(live, size=min(n, len(live)), replace=False)]   # most are not in the query: stale or other stamp
    return neighbours


MAPS = {"same": lambda h: 0, "other": lambda h: 1, "mixed": lambda h: h % 3, "bad": lambda h: h % 3}


@pytest.mark.parametrize("name", ["three_queries", "interleaved", "erase_between", "order_41", "db_300", "growth"])
def test_selection_matches_the_restatement(ctx, name):
    ref = kr.KeyFrameDatabase()
    ref_ops = iter(kc.ops(name))
    seen = {"loop": 0, "merge": 0, "reloc": 0, "moved": 0}

    def after_query(db, k, op, got, e):
        for o in ref_ops:                               # the restatement's database up to the same query
            kc.replay(ref, o)
            if o is op:
                break
        kind, qid = op[1], op[2]
        for mode in ("none", "some"):
            neighbours = _neighbours_of(e["live"], 100 + k, mode)
            for mname, maps in MAPS.items():
                bad = (2,) if mname == "bad" else ()
                if kind == PLACE:
                    for n_cand in (1, 3, 1000):
                        want = ref.select_n_best(qid, e["result"], neighbours, maps, 0, n_cand, bad)
                        have = db.select_n_best(qid, got, neighbours, maps, 0, n_cand, bad)
                        assert [h.tolist() for h in have] == [list(w) for w in want], (name, k, mode, mname, n_cand)
                        seen["loop"] += len(want[0])
                        seen["merge"] += len(want[1])
                    acc, _ = ref._accumulate(PLACE, qid, e["result"], neighbours)
                    seen["moved"] += sum(b != int(h) for (_, b), h in zip(acc, e["result"]["handles"]))
                else:
                    want = ref.select_reloc(qid, e["result"], neighbours, maps, 0)
                    have = db.select_reloc(qid, got, neighbours, maps, 0)
                    assert have.tolist() == list(want), (name, k, mode, mname)
                    seen["reloc"] += len(want)
    _replay(ctx, name, after_query)
    assert seen["loop"] and seen["merge"], seen
    if name in ("interleaved", "erase_between", "order_41", "db_300", "growth"):
        assert seen["reloc"], seen
    if name in ("three_queries", "order_41"):
        assert seen["moved"], seen                      # a neighbour outscored its keyframe somewhere: pBestKF moved, duplicates follow


def test_selection_hand_cases(ctx):
    db = orb.KeyFrameDatabase(ctx)
    one = (np.array([1, 2, 3], np.uint32), np.array([0.5, 0.25, 0.25]))
    hs = db.add([one] * 4)
    r = db.score(PLACE, 1, *one)
    assert r["handles"].tolist() == hs.tolist() and len(set(r["scores"].tolist())) == 1
    # equal accumulated scores keep list order (a stable sort), and the walk stops when both lists are full
    loop, merge = db.select_n_best(1, r, lambda h: [], lambda h: h % 2, 0, 1)
    assert loop.tolist() == [0] and merge.tolist() == [1]
    loop, merge = db.select_n_best(1, r, lambda h: [], lambda h: h % 2, 0, 10)
    assert loop.tolist() == [0, 2] and merge.tolist() == [1, 3]
    loop, merge = db.select_n_best(1, r, lambda h: [], lambda h: 0, 1, 10, bad_maps=[0])     # every candidate in a bad other map
    assert loop.tolist() == [] and merge.tolist() == []
    loop, merge = db.select_n_best(1, r, lambda h: [], lambda h: 0, 1, 0)
    assert loop.tolist() == [] and merge.tolist() == []
    # the relocalisation boundary: 0.75f * best is not retained, the next float is
    rr = db.score(RELOC, 9, *one)
    scored = dict(handles=rr["handles"][:3], scores=np.array([1.0, 0.75, np.nextafter(np.float32(0.75), np.float32(1))], np.float32))
    assert db.select_reloc(9, scored, lambda h: [], lambda h: 0, 0).tolist() == [0, 2]
    assert db.select_reloc(9, scored, lambda h: [], lambda h: 1 if h == 0 else 0, 0).tolist() == [2]
    # a neighbour counts with its stored score only under this query's stamp
    # (2.0, 1.75 and the float above pass 1.5; keyframe 3 outscores 1 and 2 and stands for both, once)
    assert db.select_reloc(9, scored, lambda h: [3], lambda h: 0, 0).tolist() == [0, 3]
    assert db.select_reloc(8, scored, lambda h: [3], lambda h: 0, 0).tolist() == [0, 2]
    db.close()


def test_end_to_end_vectors_of_a_vocabulary(ctx):
    voc = synth.make_vocabulary(10, 4, seed=5)
    gv = orb.Vocabulary(ctx, 10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["descriptors"], voc["weights"])
    rng = np.random.default_rng(11)
    leaves = voc["descriptors"][np.nonzero(voc["is_leaf"])[0]]
    place = leaves[rng.choice(len(leaves), 300, replace=False)]          # a place: 300 words; views of it see 70 % of them
    vectors = []
    for k in range(40):
        d = np.concatenate([place[rng.random(300) < 0.7], leaves[rng.choice(len(leaves), 150)]])
        t = gv.transform(d, 4)
        vectors.append((t["bow_ids"].copy(), t["bow_values"].copy()))
    db, ref = orb.KeyFrameDatabase(ctx), kr.KeyFrameDatabase()
    assert db.add(vectors[:39]).tolist() == [ref.add(*v) for v in vectors[:39]]
    q = vectors[39]
    for kind, qid, conn in ((PLACE, 39, [37, 38]), (RELOC, 1, []), (PLACE, 40, [])):
        want, got = ref.score(kind, qid, *q, conn), db.score(kind, qid, *q, conn)
        _same_result(got, want, (kind, qid))
        assert want["n_sharing"] >= 30 and len(want["handles"]) >= 3
    live = list(range(39))
    for kind in (PLACE, RELOC):
        for g, w in zip(db.state(kind, live), ref.state(kind, live)):
            assert np.array_equal(_bits(g), _bits(w))
    neighbours, maps = _neighbours_of(live, 7, "some"), (lambda h: h // 20)
    got = db.DetectNBestCandidates(41, *q, [38], neighbours, maps, 1, 3)
    want = ref.select_n_best(41, ref.score(PLACE, 41, *q, [38]), neighbours, maps, 1, 3)
    assert [g.tolist() for g in got] == [list(w) for w in want]
    got = db.DetectRelocalizationCandidates(2, *q, neighbours, maps, 0)
    assert got.tolist() == list(ref.select_reloc(2, ref.score(RELOC, 2, *q), neighbours, maps, 0))
    db.close()
    gv.close()


def test_errors(ctx):
    L = _capi.lib()
    INVALID, CAPACITY = _capi.FT_ERR_INVALID, _capi.FT_ERR_CAPACITY

    def err(word):
        assert word in L.ft_last_error().decode(), L.ft_last_error()

    h = C.c_void_p()
    assert L.ft_kfdb_create(ctx._h, 1, C.byref(h)) == INVALID            # L2_NORM
    err("L1_NORM")
    assert L.ft_kfdb_create(None, 0, C.byref(h)) == INVALID
    db = orb.KeyFrameDatabase(ctx)
    v = kc.make_vector(np.random.default_rng(0), 256, 40)
    hs = db.add([v, v, v])
    p = _capi.ptr
    out = np.zeros(8, np.int32)
    # add: ids not strictly ascending, null arrays with words, bad offsets
    assert L.ft_kfdb_add(db._h, 1, p(np.array([0, 2], np.int32)), p(np.array([5, 5], np.uint32)), p(np.ones(2)), p(out)) == INVALID
    err("strictly ascending")
    assert L.ft_kfdb_add(db._h, 1, p(np.array([0, 2], np.int32)), None, p(np.ones(2)), p(out)) == INVALID
    assert L.ft_kfdb_add(db._h, 1, p(np.array([1, 2], np.int32)), p(np.array([5, 6], np.uint32)), p(np.ones(2)), p(out)) == INVALID
    assert db.size()[0] == 3
    # erase: unknown, already erased, twice in one call - and nothing is erased by a refused call
    for bad in ([7], [-1], [0, 0], [1, 99]):
        with pytest.raises(_capi.FastTrackError) as e:
            db.erase(bad)
        assert e.value.status == INVALID
    assert db.size()[0] == 3
    db.erase([1])
    with pytest.raises(_capi.FastTrackError) as e:
        db.erase([1])
    assert e.value.status == INVALID and "already erased" in str(e.value)
    # score
    ns = [C.c_int() for _ in range(4)]
    o = [np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8, np.float32), np.zeros(8, np.float64)]

    def score(kind, ids, vals, conn, n_words=None, n_conn=None):
        ids = None if ids is None else np.ascontiguousarray(ids, np.uint32)
        vals = None if vals is None else np.ascontiguousarray(vals, np.float64)
        conn = None if conn is None else np.ascontiguousarray(conn, np.int32)
        return L.ft_kfdb_score(db._h, kind, 5, len(ids) if n_words is None else n_words, p(ids), p(vals),
                               len(conn) if n_conn is None else n_conn, p(conn), *[C.byref(x) for x in ns], *[p(x) for x in o])
    assert score(PLACE, [3, 3], [0.5, 0.5], []) == INVALID
    err("strictly ascending")
    assert score(PLACE, [4, 3], [0.5, 0.5], []) == INVALID
    assert score(PLACE, v[0], v[1], [1]) == INVALID                      # an erased keyframe in the connected set
    err("not live")
    assert score(PLACE, v[0], v[1], [55]) == INVALID
    assert score(PLACE, None, None, [], n_words=3) == INVALID
    assert score(PLACE, v[0], v[1], None, n_conn=2) == INVALID
    assert score(RELOC, v[0], v[1], [0]) == INVALID                      # the relocalisation query has no connected set
    assert score(2, v[0], v[1], []) == INVALID
    big = np.arange(_capi.KFDB_MAX_QUERY_WORDS + 1, dtype=np.uint32)
    assert score(PLACE, big, np.ones(len(big)), []) == CAPACITY
    err(str(_capi.KFDB_MAX_QUERY_WORDS))
    assert (db.state(PLACE, [0, 2])[0] == 0).all()                       # no refused call touched the state
    ok = np.arange(4000, dtype=np.uint32)                                # 2 x nFeatures words fit
    assert score(PLACE, ok, np.full(4000, 1 / 4000), []) == _capi.FT_OK
    # selection: an erased or unknown handle among the scored keyframes or the neighbours
    r = db.score(PLACE, 6, *v)
    assert r["handles"].tolist() == [0, 2]
    for neighbours in (lambda h: [1], lambda h: [99]):
        with pytest.raises(_capi.FastTrackError) as e:
            db.select_n_best(6, r, neighbours, lambda h: 0, 0, 3)
        assert e.value.status == INVALID
        with pytest.raises(_capi.FastTrackError):
            db.select_reloc(6, r, neighbours, lambda h: 0, 0)
    with pytest.raises(_capi.FastTrackError):
        db.select_n_best(6, dict(handles=np.array([1], np.int32), scores=np.ones(1, np.float32)), lambda h: [], lambda h: 0, 0, 3)
    with pytest.raises(_capi.FastTrackError):
        db.state(PLACE, [1])
    # the database still answers after the errors
    want = kr.KeyFrameDatabase()
    for _ in range(3):
        want.add(*v)
    want.erase(1)
    want.score(PLACE, 5, ok, np.full(4000, 1 / 4000), [])
    want.score(PLACE, 6, *v)
    _same_result(db.score(PLACE, 7, *v, [2]), want.score(PLACE, 7, *v, [2]), "after errors")
    db.close()


def test_the_context_outlives_its_databases():
    """a database is an object of its context: the context refuses to go while one lives, and works on after the last one went"""
    ctx = orb.Context(0)
    db = orb.KeyFrameDatabase(ctx)
    v = kc.make_vector(np.random.default_rng(1), 128, 30)
    db.add([v])
    with pytest.raises(_capi.FastTrackError):
        ctx.close()
    assert ctx._h is not None
    assert db.score(PLACE, 1, *v)["handles"].tolist() == [0]
    db.close()
    d = synth.make_image(64, 64, seed=1).reshape(-1, 32)[:8]
    assert (ctx_distance(ctx, d) == 0).all()            # a call of the context after the destroy of its last object
    db2 = orb.KeyFrameDatabase(ctx)                     # and a new database starts from nothing
    assert db2.size() == (0, 0) and db2.add([v]).tolist() == [0]
    db2.close()
    ctx.close()
    assert ctx._h is None


def ctx_distance(ctx, d):
    return orb.KernelController.descriptor_distance(ctx, d, d)

"""Seeded cases of the KeyFrameDatabase queries for tests/test_kfdb_cpu.py, tests/test_gpu_kfdb.py and tests/tools/soak_kfdb.py.
A case is a list of concrete operations on one database:
    ("add", [(ids, values), ...])   ("erase", [handles])   ("clear",)
    ("query", kind, query_id, ids, values, [connected handles])
BowVectors are generated directly: sorted ids in [0, W) and L1-normalised weights with a count x idf spread, the idf from a
short table - shared words and tied values are the rule.  An operation that depends on an earlier result (erase the keyframe
that held the maximum) is made concrete by running the restatement while the case is built."""
import functools

import numpy as np

from tests import kfdb_ref as kr

PLACE, RELOC = 0, 1
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 200, 1500]   # words of a stored vector, mixed in one database
QUERY_LENGTHS = [1, 64, 65, 1500]
DB_SIZES = [0, 1, 2, 63, 64, 65, 300]
IDF = np.array([0.5, 1.0, 1.0, 2.0, 3.5, 3.5, 7.25, 12.0])


def make_vector(rng, W, n):
    n = min(n, W)
    ids = np.sort(rng.choice(W, size=n, replace=False)).astype(np.uint32)
    if n == 0:
        return ids, np.zeros(0, np.float64)
    v = rng.integers(1, 4, n).astype(np.float64) * IDF[(ids.astype(np.int64) * 2654435761 >> 7) % len(IDF)]
    return ids, v / v.sum()


def near_vector(rng, W, base_ids, keep, extra):
    """a vector that shares about `keep` of base_ids and holds `extra` other words"""
    take = base_ids[rng.random(len(base_ids)) < keep]
    other = rng.choice(W, size=extra, replace=False).astype(np.uint32)
    ids = np.unique(np.concatenate([take, other])).astype(np.uint32)
    v = rng.integers(1, 4, len(ids)).astype(np.float64) * IDF[(ids.astype(np.int64) * 2654435761 >> 7) % len(IDF)]
    return ids, v / v.sum()


class Builder:
    """collects the operations of a case and runs the restatement beside them"""

    def __init__(self, seed, W):
        self.rng = np.random.default_rng(seed)
        self.W = W
        self.ops = []
        self.ref = kr.KeyFrameDatabase()
        self.last = None

    def live(self):
        return sorted(self.ref.keyframes)

    def add(self, vectors):
        self.ops.append(("add", vectors))
        return [self.ref.add(*v) for v in vectors]

    def add_lengths(self, lengths):
        return self.add([make_vector(self.rng, self.W, n) for n in lengths])

    def erase(self, handles):
        handles = [int(h) for h in handles]
        self.ops.append(("erase", handles))
        for h in handles:
            self.ref.erase(h)

    def clear(self):
        self.ops.append(("clear",))
        self.ref.clear()

    def query(self, kind, query_id, vector, connected=()):
        connected = [int(h) for h in connected]
        self.ops.append(("query", kind, query_id, vector[0], vector[1], connected))
        self.last = self.ref.score(kind, query_id, vector[0], vector[1], connected)
        return self.last

    def some(self, fraction):
        live = self.live()
        return [h for h in live if self.rng.random() < fraction]


def _shapes(n_kf):
    b = Builder(1000 + n_kf, 4096)
    b.add_lengths([LENGTHS[(k * 7 + 3) % len(LENGTHS)] for k in range(n_kf)])
    qid = 10
    for k, nq in enumerate(QUERY_LENGTHS):
        conn = [[], b.some(0.3), b.live(), b.some(0.05)][k]
        b.query(PLACE, qid, make_vector(b.rng, b.W, nq), conn)
        b.query(RELOC, qid + 1, make_vector(b.rng, b.W, nq))
        qid += 2
    return b


def _order(seed, n_base):
    """the summation-order cases: many keyframes above the threshold, with about 16 - 20, 40 - 50 and 75 - 95 common words"""
    b = Builder(seed, 512)
    base = make_vector(b.rng, b.W, n_base)
    b.add([near_vector(b.rng, b.W, base[0], 0.55 + 0.25 * b.rng.random(), 40) for _ in range(120)])
    b.query(PLACE, 5, base)
    b.query(RELOC, 5, base)
    return b


def _three_queries():
    b = Builder(21, 1024)
    b.add_lengths([200] * 40 + [64, 65, 17, 1])
    q = make_vector(b.rng, b.W, 300)
    b.query(PLACE, 7, q, b.some(0.2))
    b.query(PLACE, 8, make_vector(b.rng, b.W, 150))       # scores of query 7 stay in the keyframes it does not score
    b.query(PLACE, 9, q, b.some(0.5))
    return b


def _repeated_id():
    b = Builder(22, 1024)
    b.add_lengths([200] * 30)
    q = make_vector(b.rng, b.W, 200)
    b.query(PLACE, 3, q)
    b.query(PLACE, 3, q)                                   # nobody is listed again, the counts accumulate
    b.query(PLACE, 3, make_vector(b.rng, b.W, 64), b.live())
    b.add_lengths([200] * 5)
    b.query(PLACE, 3, q)                                   # only the new keyframes are listed
    b.query(PLACE, 0, q)
    b.add_lengths([200] * 5)
    b.query(PLACE, 0, q)                                   # a fresh keyframe carries stamp 0: query id 0 does not list it
    b.query(RELOC, 0, q)
    return b


def _erase_between():
    b = Builder(23, 1024)
    b.add_lengths([150] * 50)
    q = make_vector(b.rng, b.W, 250)
    r = b.query(PLACE, 4, q)
    b.erase([r["handles"][int(np.argmax(r["words"]))]])    # the keyframe that held maxCommonWords
    r = b.query(PLACE, 5, q)
    b.erase(sorted(set(int(h) for h in r["handles"][:3]) | set(b.live()[:2])))
    b.query(PLACE, 6, q, b.some(0.2))
    b.query(RELOC, 6, q)
    return b


def _compaction():
    b = Builder(24, 1024)
    hs = b.add_lengths([100] * 40)
    q = make_vector(b.rng, b.W, 200)
    b.query(PLACE, 2, q)
    b.erase(hs[:15])
    b.query(PLACE, 3, q)
    b.erase(hs[15:26])                                     # 26 of 40 equal vectors are dead: more than half of the words
    b.query(PLACE, 4, q)
    b.query(RELOC, 4, q)
    b.add_lengths([100, 0, 17])
    b.query(PLACE, 5, q, b.some(0.3))
    return b


def _add_after_erase():
    b = Builder(25, 1024)
    hs = b.add_lengths([64, 65, 63, 200, 0, 16])
    q = make_vector(b.rng, b.W, 400)
    b.query(PLACE, 2, q)
    b.erase([hs[1], hs[4]])
    b.add_lengths([65, 1, 200])
    b.query(PLACE, 3, q)
    b.erase(b.live())                                      # everything goes
    b.query(PLACE, 4, q)
    b.add_lengths([17, 200])
    b.query(PLACE, 5, q)
    return b


def _growth():
    b = Builder(26, 2048)
    b.add_lengths([120] * 60)
    q = make_vector(b.rng, b.W, 500)
    b.query(PLACE, 2, q)
    b.add_lengths([120] * 80)                              # 64 -> 256 rows, 8 192 -> 32 768 words: two doublings of each
    b.query(PLACE, 3, q, b.some(0.1))
    b.erase(b.some(0.2))
    b.add_lengths([120] * 200)
    b.query(PLACE, 4, q)
    b.query(RELOC, 4, q)
    return b


def _clear():
    b = Builder(27, 512)
    b.add_lengths([64] * 20)
    q = make_vector(b.rng, b.W, 100)
    b.query(PLACE, 2, q)
    b.clear()
    b.query(PLACE, 3, q)
    b.add_lengths([64] * 5)                                # handles go on from 20
    b.query(PLACE, 3, q)
    return b


def _interleaved():
    b = Builder(28, 1024)
    b.add_lengths([200] * 40)
    q1, q2 = make_vector(b.rng, b.W, 300), make_vector(b.rng, b.W, 300)
    b.query(PLACE, 5, q1, b.some(0.2))
    b.query(RELOC, 5, q2)                                  # the same id: the kinds keep their own stamps
    b.query(PLACE, 6, q2)
    b.query(RELOC, 5, q1)
    b.query(RELOC, 7, q1)
    return b


def _hand_threshold(max_words):
    """keyframes sharing 1 .. max_words words with the query: (int)(max * 0.8f) is 4 at 5, 8 at 10, 12 at 15, and the test is >"""
    b = Builder(30 + max_words, 64)
    q_ids = np.sort(b.rng.choice(50, size=max_words, replace=False)).astype(np.uint32)
    q_v = b.rng.integers(1, 4, max_words).astype(np.float64)
    q = (q_ids, q_v / q_v.sum())
    vecs = []
    for k in range(1, max_words + 1):
        ids = np.concatenate([q_ids[:k], np.array([60, 61, 62], np.uint32)]).astype(np.uint32)   # (the query holds none of 60 - 62)
        v = np.arange(1, len(ids) + 1, dtype=np.float64)
        vecs.append((ids, v / v.sum()))
    b.add(vecs)
    b.query(PLACE, 9, q)
    b.query(RELOC, 9, q)
    return b


_CASES = {"db_%d" % n: functools.partial(_shapes, n) for n in DB_SIZES}
_CASES.update({"order_%d" % s: functools.partial(_order, s, n) for s, n in ((41, 110), (42, 60), (43, 24))})
_CASES.update({"threshold_%d" % m: functools.partial(_hand_threshold, m) for m in (5, 10, 15)})
_CASES.update(three_queries=_three_queries, repeated_id=_repeated_id, erase_between=_erase_between, compaction=_compaction,
              add_after_erase=_add_after_erase, growth=_growth, clear=_clear, interleaved=_interleaved)
NAMES = list(_CASES)
ORDER_NAMES = [n for n in NAMES if n.startswith("order_")]


@functools.lru_cache(maxsize=None)
def ops(name):
    """the operations of a case (arrays read-only)"""
    out = _CASES[name]().ops
    for op in out:
        if op[0] == "add":
            for ids, vals in op[1]:
                ids.setflags(write=False), vals.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """per operation of the case what the restatement answers: for a query dict(result, live, state) with the state of both kinds
    for every live keyframe, for an add the handles, else None.  Computed once and left unchanged."""
    ref = kr.KeyFrameDatabase()
    out = []
    for op in ops(name):
        r = replay(ref, op)
        if op[0] == "query":
            live = sorted(ref.keyframes)
            r = dict(result=r, live=live, state=[ref.state(k, live) for k in (PLACE, RELOC)])
        out.append(r)
    return out


def replay(db, op):
    """one operation on a database - the restatement or orb.KeyFrameDatabase, they answer alike"""
    if op[0] == "add":
        if isinstance(db, kr.KeyFrameDatabase):
            return [db.add(*v) for v in op[1]]
        return [int(h) for h in db.add(op[1])]
    if op[0] == "erase":
        if isinstance(db, kr.KeyFrameDatabase):
            for h in op[1]:
                db.erase(h)
        else:
            db.erase(op[1])
        return None
    if op[0] == "clear":
        db.clear()
        return None
    _, kind, qid, ids, vals, conn = op
    r = db.score(kind, qid, ids, vals, conn)
    return r


def random_case(seed, n_ops=12):
    """a random sequence for the soak: adds, erasures and queries of both kinds on one database"""
    b = Builder(seed, int(np.random.default_rng(seed).choice([64, 256, 1024, 4096])))
    rng = b.rng
    b.add_lengths(rng.choice(LENGTHS[:9], size=int(rng.integers(0, 80))))
    qid = 1
    for _ in range(n_ops):
        what = rng.random()
        if what < 0.2:
            b.add_lengths(rng.choice(LENGTHS[:9], size=int(rng.integers(1, 40))))
        elif what < 0.4 and b.live():
            b.erase(b.some(rng.choice([0.05, 0.3, 0.7])))
        elif what < 0.43:
            b.clear()
        else:
            kind = int(rng.integers(0, 2))
            base = make_vector(rng, b.W, int(rng.choice([1, 16, 64, 65, 200, 400])))
            b.query(kind, qid, base, b.some(0.2) if kind == PLACE else ())
            qid += int(rng.integers(0, 2))
    return b.ops

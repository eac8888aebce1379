"""Hand-built calls of ft_distinctive_descriptors (MapPoint::ComputeDistinctiveDescriptors, reference src/MapPoint.cc:329-403), used
by the CPU test (the restatement against an independent formulation and against the answers worked out here) and by the GPU test (the
library against the restatement).  A case is one call: dict(name, lists = the vDescriptors of every point, and where the answer is
worked out by hand: index / median per point)."""
import functools

import numpy as np

CAP = 1024  # FT_DISTINCT_MAX_OBSERVATIONS (include/fasttrack_amd.h)


def line(*positions):
    """Descriptors on a line: the one at position t has its first t bits set, so d(i, j) = |t_i - t_j| (0 <= t <= 256)"""
    out = np.zeros((len(positions), 256), np.uint8)
    for r, t in enumerate(positions):
        out[r, :t] = 1
    return np.packbits(out, axis=1, bitorder="little")


def near(seed, n, flips=6):
    """n descriptors that are one random base with up to `flips` bits flipped each: small distances, so medians tie often"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    bits = np.tile(np.unpackbits(base), (n, 1))
    for r in range(n):
        k = int(rng.integers(0, flips + 1))
        pos = rng.choice(256, size=k, replace=False)
        bits[r, pos] ^= 1
    return np.packbits(bits, axis=1)


def spread(seed, n):
    """n independent random descriptors (distances around 128)"""
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


EMPTY = np.zeros((0, 32), np.uint8)


def pack(lists):
    """-> (obs_offsets [P + 1] int32, descriptors [total, 32] uint8)"""
    offsets = np.zeros(len(lists) + 1, np.int32)
    offsets[1:] = np.cumsum([len(v) for v in lists])
    desc = np.concatenate([np.asarray(v, np.uint8).reshape(-1, 32) for v in lists] + [EMPTY])
    return offsets, np.ascontiguousarray(desc)


def _case(name, lists, index=None, median=None):
    c = dict(name=name, lists=[np.asarray(v, np.uint8).reshape(-1, 32) for v in lists])
    if index is not None:
        c["index"], c["median"] = list(index), list(median)
        assert len(index) == len(median) == len(lists)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    A = spread(1, 1)
    notA = np.bitwise_not(A)
    B = A.copy()
    B[0, :10] ^= 1  # ten bits of A flipped: d(A, B) = 10, d(~A, B) = 246
    tie = line(40, 0, 4)  # d = |difference|: rows [0 40 36], [40 0 4], [36 4 0] -> medians 36, 4, 4
    mixed = [near(20, 2), near(21, 5), near(22, 8), near(23, 11), near(24, 16), near(25, 30), spread(26, 64), near(27, 90), near(28, 3)]
    long_one = near(29, 200, flips=40)
    out = [
        # the median index (size_t)(0.5 * (N - 1)) goes 0, 0, 1, 1, 2 for N = 1 .. 5: the LOWER median of N = 2 and 4.
        #   N = 1: the diagonal.  N = 2: both rows sort to [0, 50] -> 0, 0 (an upper median would answer 50).
        #   N = 3 at 0, 100, 110: [0 100 110], [0 10 100], [0 10 110] -> 100, 10, 10: the first of the two.
        #   N = 4 at 0, 10, 30, 100: [0 10 30 100], [0 10 20 90], [0 20 30 70], [0 70 90 100] -> 10, 10, 20, 70 (upper: 30, 20, 30, 90)
        #   N = 5 at 0, 200, 90, 100, 120: [0 90 100 120 200], [0 80 100 110 200], [0 10 30 90 110], [0 10 20 100 100],
        #                                  [0 20 30 80 120] -> 100, 100, 30, 20, 30
        _case("median_index_1_to_5", [line(7), line(0, 50), line(0, 100, 110), line(0, 10, 30, 100), line(0, 200, 90, 100, 120)],
              index=[0, 0, 1, 0, 3], median=[0, 0, 10, 10, 20]),
        _case("subgroup_edges", [near(30 + n, n) for n in (7, 8, 9, 15, 16, 17)]),
        _case("subgroup_edges_spread", [spread(40 + n, n) for n in (7, 8, 9, 15, 16, 17)]),
        _case("wave_edges", [near(50 + n, n, flips=12) for n in (63, 64, 65)]),
        _case("wave_edges_spread", [spread(60 + n, n) for n in (63, 64, 65)]),
        _case("n300", [near(70, 300, flips=30)]),
        _case("cap", [near(71, CAP, flips=60)]),
        # every descriptor equal: all medians 0, the strict < keeps index 0
        _case("all_equal", [np.repeat(A, 5, axis=0), np.repeat(B, 16, axis=0), np.repeat(A, 40, axis=0), np.repeat(B, 100, axis=0)],
              index=[0, 0, 0, 0], median=[0, 0, 0, 0]),
        # a descriptor and its complement are 256 apart.  N = 2: both medians are the diagonal.  N = 3, (A, ~A, ~A): rows [0 256 256],
        # [256 0 0], [256 0 0] -> 256, 0, 0: a distance kept in a byte would turn row 0 into zeros and answer index 0.
        # (A, ~A, B): [0 256 10], [256 0 246], [10 246 0] -> 10, 246, 10.  (~A, A, B): 246, 10, 10.
        _case("complement", [np.concatenate([A, notA]), np.concatenate([A, notA, notA]), np.concatenate([A, notA, B]),
                             np.concatenate([notA, A, B])], index=[0, 1, 0, 1], median=[0, 0, 10, 10]),
        # a worse row, then two rows with the same smallest median: the first of them (a = 1, not b = 2) ...
        _case("tie", [tie], index=[1], median=[4]),
        # ... and the same list reversed: rows [0 4 36], [4 0 40], [36 40 0] -> 4, 4, 36: index 0, which is the OTHER descriptor
        _case("tie_reversed", [tie[::-1]], index=[0], median=[4]),
        _case("empty_first", [EMPTY, near(80, 4), near(81, 20)]),
        _case("empty_middle", [near(82, 6), EMPTY, EMPTY, near(83, 70)]),
        _case("empty_last", [near(84, 9), near(85, 2), EMPTY]),
        _case("all_empty", [EMPTY, EMPTY, EMPTY], index=[-1, -1, -1], median=[-1, -1, -1]),
        _case("no_points", []),
        _case("one_point", [near(86, 6)]),
        _case("mixed_long_first", [long_one] + mixed),
        _case("mixed_long_last", mixed + [long_one]),
        # 300 points of two observations: one class only, more than a workgroup's worth of sub-groups
        _case("many_short", [near(1000 + p, 2, flips=3) for p in range(300)], index=[0] * 300, median=[0] * 300),
    ]
    assert len({c["name"] for c in out}) == len(out)
    return out


def by_name(name):
    return next(c for c in cases() if c["name"] == name)

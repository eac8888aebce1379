"""The restatement of MapPoint::ComputeDistinctiveDescriptors (tests/distinct_ref.py) against what is known without a GPU: an
independent numpy formulation, the answers worked out by hand in tests/distinct_cases.py, the median index - and the library's
export of ft_distinctive_descriptors."""
import numpy as np

from fasttrack_amd import _capi
from tests import distinct_cases as dc
from tests import distinct_ref as dr


def independent(v):
    """the lower median of every row of the full distance matrix, then the first argmin"""
    v = np.asarray(v, np.uint8).reshape(-1, 32)
    N = len(v)
    if N == 0:
        return -1, -1
    bits = np.unpackbits(v, axis=1).astype(np.int32)
    D = bits @ (1 - bits).T + (1 - bits) @ bits.T
    med = np.sort(D, axis=1)[:, (N - 1) // 2]
    i = int(np.argmin(med))
    return i, int(med[i])


def test_restatement_equals_the_independent_formulation_on_every_case():
    for c in dc.cases():
        for p, v in enumerate(c["lists"]):
            assert dr.compute_distinctive_descriptor(v) == independent(v), (c["name"], p)


def test_restatement_equals_the_independent_formulation_on_random_lists():
    rng = np.random.default_rng(2024)
    ties = 0
    for t in range(300):
        n = int(rng.integers(1, 81))
        v = dc.near(5000 + t, n, flips=int(rng.integers(1, 9))) if t % 3 else dc.spread(5000 + t, n)
        got = dr.compute_distinctive_descriptor(v)
        assert got == independent(v), (t, n)
        D = np.array(dr.distance_matrix(v))
        med = np.sort(D, axis=1)[:, (n - 1) // 2]
        ties += int((med == med.min()).sum() > 1)
    assert ties > 100  # the flipped-bit lists do make the smallest median a tie


def test_the_two_distance_paths_of_the_restatement_agree():
    v = dc.near(9, 32, flips=20)
    small = dr.distance_matrix(v)                       # the loops as written
    big = dr.distance_matrix(np.concatenate([v, v]))    # the popcount table
    assert np.array_equal(np.array(big)[:32, :32], np.array(small)) and np.array_equal(np.array(big)[32:, :32], np.array(small))


def test_median_index_is_the_lower_median_up_to_the_cap():
    for n in range(1, dc.CAP + 1):
        assert int(0.5 * (n - 1)) == (n - 1) // 2, n
    assert [int(0.5 * (n - 1)) for n in (1, 2, 3, 4, 5)] == [0, 0, 1, 1, 2]


def test_hand_computed_answers():
    seen = 0
    for c in dc.cases():
        if "index" not in c:
            continue
        offsets, desc = dc.pack(c["lists"])
        idx, med, out = dr.distinctive_descriptors(offsets, desc)
        assert idx.tolist() == c["index"] and med.tolist() == c["median"], (c["name"], idx.tolist(), med.tolist())
        for p, v in enumerate(c["lists"]):
            assert np.array_equal(out[p], v[idx[p]] if len(v) else np.zeros(32, np.uint8)), (c["name"], p)
        seen += 1
    assert seen >= 7
    # the reversed tie resolves to a different descriptor
    f, r = dc.by_name("tie"), dc.by_name("tie_reversed")
    assert not np.array_equal(f["lists"][0][f["index"][0]], r["lists"][0][r["index"][0]])


def test_cases_cover_the_length_classes():
    lengths = {len(v) for c in dc.cases() for v in c["lists"]}
    assert {0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 300, dc.CAP} <= lengths
    assert dc.CAP == _capi.DISTINCT_MAX_OBSERVATIONS >= 1024
    text = open(_capi.HEADER_PATH).read()
    assert "#define FT_DISTINCT_MAX_OBSERVATIONS %d\n" % dc.CAP in text


def test_library_exports_the_entry_point():
    assert "ft_distinctive_descriptors" in _capi.declared_symbols()
    L = _capi.lib()
    assert hasattr(L, "ft_distinctive_descriptors")
    assert len(L.ft_distinctive_descriptors.argtypes) == 7

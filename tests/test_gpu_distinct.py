"""ft_distinctive_descriptors on the device against the sequential restatement of MapPoint::ComputeDistinctiveDescriptors
(tests/distinct_ref.py): best_index, best_median and the 32 bytes equal, no tolerance and no excluded case.  Needs an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

from fasttrack_amd import _capi, orb
from tests import distinct_cases as dc
from tests import distinct_ref as dr

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
NAMES = [c["name"] for c in dc.cases()]


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's answer for a case, computed once; the rows of points with an empty list hold the sentinel"""
    c = dc.by_name(name)
    offsets, desc = dc.pack(c["lists"])
    idx, med, out = dr.distinctive_descriptors(offsets, desc, np.full((len(c["lists"]), 32), SENTINEL, np.uint8))
    for a in (idx, med, out):
        a.setflags(write=False)
    return idx, med, out


def run(ctx, lists, **kw):
    offsets, desc = dc.pack(lists)
    return ctx.distinctive_descriptors(offsets, desc, np.full((max(len(lists), 1), 32), SENTINEL, np.uint8), **kw)


@pytest.mark.parametrize("name", NAMES)
def test_cases_match_the_restatement(ctx, name):
    c = dc.by_name(name)
    want = expected(name)
    idx, med, out = run(ctx, c["lists"])
    assert np.array_equal(idx, want[0]), (name, np.nonzero(idx != want[0])[0][:10], idx[:10], want[0][:10])
    assert np.array_equal(med, want[1]), (name, np.nonzero(med != want[1])[0][:10], med[:10], want[1][:10])
    assert np.array_equal(out, want[2]), name
    for p, v in enumerate(c["lists"]):
        if len(v) == 0:  # the reference returns at :365 without touching mDescriptor
            assert idx[p] == -1 and med[p] == -1 and (out[p] == SENTINEL).all(), (name, p)
    if "index" in c:
        assert idx.tolist() == c["index"] and med.tolist() == c["median"], name


@pytest.mark.parametrize("name", NAMES)
def test_optional_outputs_may_be_null(ctx, name):
    c = dc.by_name(name)
    idx, med, out = run(ctx, c["lists"], want_median=False, want_descriptors=False)
    assert med is None and out is None
    assert np.array_equal(idx, expected(name)[0]), name


@pytest.mark.parametrize("name", ["mixed_long_first", "mixed_long_last", "empty_middle"])
def test_points_do_not_depend_on_their_call(ctx, name):
    c = dc.by_name(name)
    idx, med, out = run(ctx, c["lists"])
    for p, v in enumerate(c["lists"]):
        i1, m1, o1 = run(ctx, [v])
        assert (int(i1[0]), int(m1[0])) == (int(idx[p]), int(med[p])), (name, p)
        assert np.array_equal(o1[0], out[p]), (name, p)


def _launches(ctx, lists):
    ctx.reset_stats()
    run(ctx, lists)
    total, calls = ctx.get_stat("distinctive_descriptors.launches")
    assert calls == 1
    return total


@pytest.mark.parametrize("name", ["mixed_long_first", "subgroup_edges", "wave_edges", "one_point", "empty_first", "many_short"])
def test_launch_count_does_not_depend_on_the_number_of_points(ctx, name):
    lists = dc.by_name(name)["lists"]
    try:
        ctx.set_kernel_timing(True)
        once = _launches(ctx, lists)
        many = _launches(ctx, [v for v in lists for _ in range(50)])
        assert once == many and 1 <= once <= 3, (name, once, many)
        ctx.reset_stats()
        idx, med, out = run(ctx, [v for v in lists for _ in range(50)])
        want = expected(name)
        assert np.array_equal(idx, np.repeat(want[0], 50)) and np.array_equal(med, np.repeat(want[1], 50))
        assert np.array_equal(out, np.repeat(want[2], 50, axis=0))
        kernels = sum(ctx.get_stat("kernel.distinct_" + k)[1] for k in ("short", "wave", "block"))
        assert kernels == ctx.get_stat("distinctive_descriptors.launches")[0] == once
    finally:
        ctx.set_kernel_timing(False)


def test_a_mixed_call_takes_three_launches(ctx):
    assert _launches(ctx, dc.by_name("mixed_long_last")["lists"]) == 3.0
    assert _launches(ctx, dc.by_name("many_short")["lists"]) == 1.0
    assert _launches(ctx, dc.by_name("cap")["lists"]) == 1.0


@pytest.mark.parametrize("name", ["all_empty", "no_points"])
def test_empty_calls_return_without_a_launch(ctx, name):
    c = dc.by_name(name)
    try:
        ctx.set_kernel_timing(True)
        ctx.reset_stats()
        idx, med, out = run(ctx, c["lists"])
        assert ctx.get_stat("distinctive_descriptors.launches") == (0.0, 0)
        assert ctx.get_stat("distinctive_descriptors.total") == (0.0, 0)
    finally:
        ctx.set_kernel_timing(False)
    assert (idx == -1).all() and (med == -1).all() and (out == SENTINEL).all() and len(idx) == len(c["lists"])


def _raw(ctx, n_points, offsets, desc, idx, med, out):
    def p(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)
    return _capi.lib().ft_distinctive_descriptors(ctx._h if ctx is not None else None, n_points, p(offsets), p(desc), p(idx), p(med), p(out))


def test_errors_leave_the_outputs_untouched(ctx):
    lists = dc.by_name("empty_middle")["lists"]
    offsets, desc = dc.pack(lists)
    n = len(lists)

    def call(status, word=None, ctx_=ctx, n_points=n, offsets_=offsets, desc_=desc, no_index=False):
        idx, med = np.full(max(n_points, n), 77, np.int32), np.full(max(n_points, n), 78, np.int32)
        out = np.full((max(n_points, n), 32), SENTINEL, np.uint8)
        rc = _raw(ctx_, n_points, offsets_, desc_, None if no_index else idx, med, out)
        assert rc == status, (rc, status, word)
        assert (idx == 77).all() and (med == 78).all() and (out == SENTINEL).all()
        if word is not None:
            assert word in _capi.lib().ft_last_error().decode(), _capi.lib().ft_last_error()

    INVALID, CAPACITY = _capi.FT_ERR_INVALID, _capi.FT_ERR_CAPACITY
    call(INVALID, ctx_=None)
    call(INVALID, offsets_=None)
    call(INVALID, no_index=True)
    call(INVALID, desc_=None)                                        # descriptors null while obs_offsets[n_points] > 0
    call(INVALID, n_points=-1)
    first = offsets.copy()
    first[0] = 1
    call(INVALID, offsets_=first)                                    # obs_offsets[0] != 0
    down = offsets.copy()
    down[2] = down[1] - 1
    call(INVALID, "point 1", offsets_=down)                          # a decreasing offset
    # a list of cap + 1, the middle one of three points: the point is named
    long_lists = [dc.near(1, 3), dc.near(2, dc.CAP + 1), dc.near(3, 3)]
    lo, ld = dc.pack(long_lists)
    call(CAPACITY, "point 1", n_points=3, offsets_=lo, desc_=ld)
    # an arena beyond 4 GB: 200 000 lists of 1 000 descriptors are 6.4 GB.  The offsets are checked before a descriptor is read, so
    # the few rows passed here are never touched.
    big = (np.arange(200001, dtype=np.int64) * 1000).astype(np.int32)
    call(CAPACITY, "4 GB", n_points=200000, offsets_=big, desc_=desc)
    # descriptors may be null when every list is empty, and the cap itself is no error
    idx, med, out = ctx.distinctive_descriptors(np.zeros(4, np.int32), np.zeros((0, 32), np.uint8))
    assert idx.tolist() == med.tolist() == [-1, -1, -1]
    want = expected("empty_middle")
    got = run(ctx, lists)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))     # the context still works after the errors

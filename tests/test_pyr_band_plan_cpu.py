"""The band plan of the one-launch pyramid (k_pyr_cascade, option pyr_rows = 2), checked on the host through ft_pyramid_band_plan.

An image is cut into K horizontal bands and one workgroup builds one band of one image through all levels without looking at
any other workgroup's rows.  That only works if, at every level, a band's row range (a) together with the other bands' covers
the level and (b) contains every source row its range one level up is resized from.  Both are checked here against the y taps
of cv::resize restated in Python (the same float arithmetic as the oracle's and the library's tap tables), for the shapes of
tests/test_gpu_pyr_cascade.py and K in {1, 2, 4, 8, top level's height + 3}.
"""
import numpy as np
import pytest

from fasttrack_amd import _capi
from oracle import binding as ob

SHAPES = [(333, 257, 1.2, 8), (1000, 96, 1.2, 2), (641, 479, 1.5, 5), (512, 512, 2.0, 4), (97, 83, 1.1, 6), (1279, 717, 1.25, 8),
          (406, 302, 2.4, 3), (300, 200, 3.0, 2), (1280, 720, 1.2, 8), (752, 480, 1.2, 8), (512, 512, 1.2, 8)]


def _plan(w, h, sf, levels, K):
    first, end = np.full(levels * K, -7, np.int32), np.full(levels * K, -7, np.int32)
    assert _capi.lib().ft_pyramid_band_plan(w, h, sf, levels, K, _capi.ptr(first), _capi.ptr(end)) == 0
    return first.reshape(levels, K), end.reshape(levels, K)


def _source_rows(hs, hd, area2x):
    """(sy0, sy1) of every row of a level of height hd made from one of height hs: cv::resize's two row taps, clipped"""
    d = np.arange(hd)
    if area2x:
        return 2 * d, 2 * d + 1
    scale = 1.0 / (float(hd) / float(hs))
    s = np.floor(((d + 0.5) * scale - 0.5).astype(np.float32)).astype(np.int64)
    return np.clip(s, 0, hs - 1), np.clip(s + 1, 0, hs - 1)


def _sizes(w, h, sf, levels):
    lw, lh = ob.level_sizes(w, h, sf, levels)
    return [int(v) for v in lw], [int(v) for v in lh]


def _expected(lw, lh, K):
    """the rule of the plan, restated: own rows, widened going down from the top by the source rows of the range above"""
    L = len(lh)
    first, end = np.zeros((L, K), np.int64), np.zeros((L, K), np.int64)
    for k in range(K):
        lo = hi = 0
        for l in range(L - 1, 0, -1):
            a, b = k * lh[l] // K, (k + 1) * lh[l] // K
            if hi > lo:
                sy0, sy1 = _source_rows(lh[l], lh[l + 1], lw[l] == 2 * lw[l + 1] and lh[l] == 2 * lh[l + 1])
                s0, s1 = int(sy0[lo]), int(sy1[hi - 1]) + 1
                a, b = (min(a, s0), max(b, s1)) if b > a else (s0, s1)
            first[l, k], end[l, k] = lo, hi = a, b
    return first, end


@pytest.mark.parametrize("w,h,sf,levels", SHAPES)
def test_bands_cover_every_level_and_read_only_their_own_rows(w, h, sf, levels):
    lw, lh = _sizes(w, h, sf, levels)
    for K in (1, 2, 4, 8, lh[-1] + 3):
        first, end = _plan(w, h, sf, levels, K)
        assert (first[0] == 0).all() and (end[0] == 0).all()
        assert (first[1:] >= 0).all() and (end[1:] >= first[1:]).all()
        for l in range(1, levels):
            assert (end[l] <= lh[l]).all()
            covered = np.zeros(lh[l], bool)
            for k in range(K):
                covered[first[l, k]:end[l, k]] = True
                a, b = k * lh[l] // K, (k + 1) * lh[l] // K  # the rows the band owns
                assert b == a or (first[l, k] <= a and b <= end[l, k])
            assert covered.all(), f"K {K} level {l}: rows {np.flatnonzero(~covered)[:5]} are nobody's"
        for l in range(2, levels):  # level l is made of level l - 1 (level 1 of the caller's frame: no constraint)
            sy0, sy1 = _source_rows(lh[l - 1], lh[l], lw[l - 1] == 2 * lw[l] and lh[l - 1] == 2 * lh[l])
            for k in range(K):
                if end[l, k] > first[l, k]:
                    rows = slice(first[l, k], end[l, k])
                    assert sy0[rows].min() >= first[l - 1, k] and sy1[rows].max() < end[l - 1, k], f"K {K} level {l} band {k}"


@pytest.mark.parametrize("w,h,sf,levels", SHAPES)
def test_empty_bands_leave_the_others_alone(w, h, sf, levels):
    """More bands than the top level has rows: some own nothing there.  Such a band is reported as first == end (the kernel runs no
    strip for it and still passes the level's barrier with its workgroup - the count of barriers is the number of levels for
    every workgroup, whatever its ranges), it may pick up rows further down, and every band's ranges are exactly what the rule
    gives for that band alone."""
    lw, lh = _sizes(w, h, sf, levels)
    K = lh[-1] + 3
    first, end = _plan(w, h, sf, levels, K)
    assert (end[levels - 1] == first[levels - 1]).sum() >= 3
    assert (end[levels - 1] > first[levels - 1]).sum() == lh[-1]  # one row each
    for K in (1, 2, 4, 8, K):
        first, end = _plan(w, h, sf, levels, K)
        wf, we = _expected(lw, lh, K)
        assert np.array_equal(first, wf) and np.array_equal(end, we)
        assert (first[1:][end[1:] == first[1:]] >= 0).all()


def test_ranges_of_the_bench_geometry():
    first, end = _plan(1280, 720, 1.2, 8, 4)
    assert [(int(first[l, 1]), int(end[l, 1])) for l in range(1, 8)] == [(147, 300), (123, 250), (103, 208), (86, 173), (72, 144),
                                                                          (60, 120), (50, 100)]
    # rows computed twice, as a share of the pyramid's pixels (levels 1 .. 7)
    lw, lh = _sizes(1280, 720, 1.2, 8)
    for K, pct in ((2, 0.2), (4, 1.9), (8, 5.2)):
        f, e = _plan(1280, 720, 1.2, 8, K)
        done = sum(int((e[l] - f[l]).sum()) * lw[l] for l in range(1, 8))
        need = sum(lh[l] * lw[l] for l in range(1, 8))
        assert abs(100.0 * (done - need) / need - pct) < 0.06, (K, 100.0 * (done - need) / need)


def test_bad_arguments():
    L = _capi.lib()
    a = np.zeros(64, np.int32)
    assert L.ft_pyramid_band_plan(640, 480, 1.2, 8, 0, _capi.ptr(a), _capi.ptr(a)) == _capi.FT_ERR_INVALID
    assert L.ft_pyramid_band_plan(640, 480, 1.0, 8, 4, _capi.ptr(a), _capi.ptr(a)) == _capi.FT_ERR_INVALID
    assert L.ft_pyramid_band_plan(640, 480, 1.2, 8, 4, None, _capi.ptr(a)) == _capi.FT_ERR_INVALID

"""k_fast_cells<TP, false>: the columns behind the 32-column halves of a cell (the remainder bands) against the oracle.

Small images whose cells sit on the edges of the packed remainder pass: every remainder width from 1 to 10 and wide
ones at the 64-byte pitch, cell heights on both sides of a multiple of 4 and of 8, last cell columns of 32 or fewer
pixels (no remainder at all).  Two levels at a scale factor of 1.05 keep both levels on a fixed-pitch variant; the geometry
test derives every cell's tested size from the extractor's own level sizes and fails if a shape left the fixed pitch.
Candidates are compared as sorted (x, y, score) rows, keypoints and descriptors bit-exactly (needs an MI355X).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from fasttrack_amd import orb, synth
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF, LEVELS, NF = 1.05, 2, 300
SHAPES = [(110, 110), (112, 126), (139, 180), (200, 166), (180, 200)]
# tested sizes of the cells along an axis of the given length (level 0), worked out by hand from ORBextractor.cc:1119-1155
LEVEL0 = {110: (39, [39, 33]), 112: (40, [40, 34]), 126: (47, [47, 41]), 139: (36, [36, 36, 29]), 166: (45, [45, 45, 38]),
          180: (37, [37, 37, 37, 31]), 200: (42, [42, 42, 42, 36])}


def _axis(size):
    """(cell size, tested size of every cell) along an axis of a level: borders of 16 px, cells of 35 px or more, every
    cell's sub-image overlaps the next by 6 px and the last ends at the border"""
    wd = size - 32
    n = wd // 35
    cell = -(-wd // n)
    return cell, [cell] * (n - 1) + [wd - (n - 1) * cell - 6]


def _cells(ex, level):
    """[(x0, y0, pw, ph)] of the level's cells: first tested pixel in level coordinates and the tested size"""
    lw, lh = ex.level_size(level)
    (cw, ws), (ch, hs) = _axis(lw), _axis(lh)
    return [(16 + j * cw + 3, 16 + i * ch + 3, pw, ph) for i, ph in enumerate(hs) for j, pw in enumerate(ws)], cw, ch


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    assert c.get_option("device_octree") != 0, "the unordered FAST variant runs in front of the device octree only"
    yield c
    c.close()


def _check_same(gk, gd, ok, od):
    assert len(gk) == len(ok)
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        assert np.array_equal(gk[f], ok[f]), f
    assert np.allclose(gk["angle"], ok["angle"], rtol=0, atol=1e-4)
    assert np.array_equal(gk["angle"], ok["angle"]), "angles agree to 1e-4 but not bit-exactly"
    assert np.array_equal(gd, od)


def _sorted_rows(c):
    c = np.asarray(c).reshape(-1, 3)
    return c[np.lexsort((c[:, 2], c[:, 0], c[:, 1]))]


def _directed(w, h, cells, which, seed):
    """flat grey with random bytes (0) in the remainder columns of every cell, every row, or (1) only in the last tested row
    and the last remainder column of every cell with one"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 128, np.uint8)
    for x0, y0, pw, ph in cells:
        if pw <= 32:
            continue
        if which == 0:
            img[y0:y0 + ph, x0 + 32:x0 + pw] = rng.integers(0, 256, (ph, pw - 32), dtype=np.uint8)
        else:
            img[y0 + ph - 1, x0:x0 + pw] = rng.integers(0, 256, pw, dtype=np.uint8)
            img[y0:y0 + ph, x0 + pw - 1] = rng.integers(0, 256, ph, dtype=np.uint8)
    return img


_ORACLE = {}


def _oracle(key, img, nf=NF, sf=SF, levels=LEVELS):
    """(keypoints, descriptors, [sorted candidates per level]) of the oracle, computed once per image"""
    if key not in _ORACLE:
        oex = ob.Extractor(nf, sf, levels)
        ok, od, _ = oex.extract(img)
        _ORACLE[key] = (ok, od, [_sorted_rows(oex.candidates(l)) for l in range(levels)])
    return _ORACLE[key]


def _images(ctx, w, h):
    """the shape's extractor and its nine images: five object scenes, two of noise, the two directed ones"""
    ex = orb.ORBextractor(ctx, NF, SF, LEVELS, 20, 7, w, h, max_batch=9)
    cells, _, _ = _cells(ex, 0)
    imgs = [synth.make_image(w, h, seed=300 + w + b) for b in range(5)]
    imgs += [synth.make_noise(w, h, seed=400 + w), synth.make_noise(w, h, seed=401 + h)]
    imgs += [_directed(w, h, cells, 0, seed=500 + w), _directed(w, h, cells, 1, seed=501 + w)]
    return ex, imgs


def _check_slots(ex, res, imgs, key, levels=LEVELS, slots=None, **okw):
    for b in (range(len(imgs)) if slots is None else slots):
        ok, od, oc = _oracle(key + (b,), imgs[b], levels=levels, **okw)
        for level in range(levels):
            gc = _sorted_rows(ex.candidates(level, b))
            assert gc.shape == oc[level].shape and np.array_equal(gc, oc[level]), f"FAST candidates of image {b}, level {level}"
        _check_same(res[b][0], res[b][1], ok, od)


def test_geometry_covers_the_edges(ctx):
    """the shapes keep every level on a fixed pitch and between them hold the remainder widths and heights the pass branches on"""
    wrem, phs, pitches, narrow = set(), set(), set(), 0
    for w, h in SHAPES:
        ex = orb.ORBextractor(ctx, NF, SF, LEVELS, 20, 7, w, h)
        assert ex.level_size(0) == (w, h)
        assert (_axis(w), _axis(h)) == (LEVEL0[w], LEVEL0[h])
        for level in range(LEVELS):
            cells, cw, ch = _cells(ex, level)
            assert cw + 9 <= 64, f"{w}x{h} level {level}: cells of {cw} columns take the any-size variant"
            pitches.add(48 if cw + 9 <= 48 else 64)
            for _, _, pw, ph in cells:
                assert 1 <= pw <= cw and 1 <= ph <= ch
                phs.add(ph)
                narrow += pw <= 32
                if pw > 32:
                    wrem.add(pw - 32)
        ex.close()
    assert {1, 2, 4, 5, 6, 7} <= wrem and max(wrem) > 8, wrem
    assert pitches == {48, 64} and narrow > 0
    assert {0, 1, 3} <= {ph % 4 for ph in phs} and {0, 1, 7} <= {ph % 8 for ph in phs}, phs


@pytest.mark.parametrize("w,h", SHAPES)
def test_single_image(ctx, w, h):
    """launches of fewer than eight images: cells dealt to the XCDs in runs"""
    ex, imgs = _images(ctx, w, h)
    for b in (0, 5, 7, 8):
        gk, gd, _ = ex.extract_batch([imgs[b]])[0]
        ok, od, oc = _oracle((w, h, b), imgs[b])
        for level in range(LEVELS):
            gc = _sorted_rows(ex.candidates(level, 0))
            assert gc.shape == oc[level].shape and np.array_equal(gc, oc[level]), f"FAST candidates of image {b}, level {level}"
        _check_same(gk, gd, ok, od)
        assert len(oc[0]) > 0  # (the directed images too: texture in the remainder columns alone yields candidates)
    ex.close()


@pytest.mark.parametrize("w,h", SHAPES)
def test_batch_of_nine(ctx, w, h):
    """eight or more images take the image -> XCD mapping; the noise images overflow the candidate ring"""
    ex, imgs = _images(ctx, w, h)
    res = ex.extract_batch(imgs)
    _check_slots(ex, res, imgs, (w, h))
    assert len(_oracle((w, h, 5), imgs[5])[2][0]) > (w - 32) * (h - 32) // 15, "the noise image no longer floods the cells"
    ex.close()


def test_headline_cells(ctx):
    """eight frames of 1280 x 720, eight levels at 1.2: the cells of the benchmark (36 to 38 columns, one trip per band)"""
    w, h, nf = 1280, 720, 2000
    imgs = [synth.make_image(w, h, seed=600 + b) for b in range(7)] + [synth.make_noise(w, h, seed=607)]
    ex = orb.ORBextractor(ctx, nf, 1.2, 8, 20, 7, w, h, max_batch=8)
    for level in range(8):
        cells, cw, _ = _cells(ex, level)
        assert cw + 9 <= 48 and {pw - 32 for _, _, pw, _ in cells if pw > 32} <= {4, 5, 6}
    res = ex.extract_batch(imgs)
    _check_slots(ex, res, imgs, (w, h), levels=8, nf=nf, sf=1.2)
    ex.close()


def test_idempotent_when_enqueued_twice():
    """FT_DEBUG_REPEAT is read once per process: a fresh child runs one shape with the FAST launch enqueued twice"""
    env = dict(os.environ, FT_DEBUG_REPEAT="fast")
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_fast_remainder"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "remainder ok, repeat 2" in r.stdout


if __name__ == "__main__":
    c_ = orb.Context(0)
    w_, h_ = SHAPES[2]
    ex_, imgs_ = _images(c_, w_, h_)
    _check_slots(ex_, ex_.extract_batch(imgs_), imgs_, (w_, h_))
    ex_.close()
    c_.close()
    print("remainder ok, repeat", 2 if "fast" in os.environ.get("FT_DEBUG_REPEAT", "") else 1)

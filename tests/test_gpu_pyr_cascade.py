"""The one-launch pyramid (k_pyr_cascade, option pyr_rows = 2, the default): a workgroup builds one horizontal band of one image
through all levels (needs an MI355X).

Launches of 8+ images whose every level fits the row-streaming strip take it; every level of EVERY slot must equal the oracle's
cv::resize chain, and keypoints and descriptors with it.  The shapes are those of test_row_streaming_pyramid_bit_exact: two levels
(no barrier inside the kernel), exact 2x (INTER_AREA, bands without overlap), bands of a few rows whose ranges overlap by more
than a strip (97 x 83 at 1.1), and scale factors 2.4 / 3.0, where a level does not fit the strip's 8-byte window and the launcher
falls back to the per-level loop.  The band plan itself is checked on the host (tests/test_pyr_band_plan_cpu.py).
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

SHAPES = [(333, 257, 1.2, 8), (1000, 96, 1.2, 2), (641, 479, 1.5, 5), (512, 512, 2.0, 4), (97, 83, 1.1, 6), (1279, 717, 1.25, 8),
          (406, 302, 2.4, 3), (300, 200, 3.0, 2)]


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def _check_batch(ctx, w, h, sf, levels, imgs, nf=300):
    with ctx.options(pyr_rows=2):
        ex = orb.ORBextractor(ctx, nf, sf, levels, 20, 7, w, h, max_batch=len(imgs))
    oex = ob.Extractor(nf, sf, levels)
    res = ex.extract_batch(imgs)
    for slot, img in enumerate(imgs):
        ok, od, om = oex.extract(img)
        for level in range(levels):
            assert np.array_equal(ex.image_pyramid_level(level, slot=slot), oex.level(level)), f"slot {slot} level {level}"
        gk, gd = res[slot][0], res[slot][1]
        assert len(gk) == len(ok)
        for f in ("x", "y", "size", "response", "octave", "class_id", "angle"):
            assert np.array_equal(gk[f], ok[f]), (slot, f)
        assert np.array_equal(gd, od), slot


@pytest.mark.parametrize("w,h,sf,levels", SHAPES)
def test_every_level_of_every_slot_bit_exact(ctx, w, h, sf, levels):
    imgs = [synth.make_image(w, h, seed=190 + b) for b in range(8)] + [synth.make_noise(w, h, seed=199)]
    _check_batch(ctx, w, h, sf, levels, imgs)


def test_bench_geometry(ctx):
    """eight frames of 1280 x 720, eight levels at 1.2: one image per XCD, four bands each"""
    w, h = 1280, 720
    imgs = [synth.make_image(w, h, seed=170 + b) if b % 2 == 0 else synth.make_noise(w, h, seed=170 + b) for b in range(8)]
    _check_batch(ctx, w, h, 1.2, 8, imgs, nf=2000)


def test_idempotent_when_enqueued_twice():
    """FT_DEBUG_REPEAT is read once per process: a fresh child runs one shape with the launch enqueued twice"""
    env = dict(os.environ, FT_DEBUG_REPEAT="pyr")
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_pyr_cascade"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "cascade ok, repeat 2" in r.stdout


if __name__ == "__main__":
    c_ = orb.Context(0)
    w_, h_, sf_, levels_ = SHAPES[0]
    _check_batch(c_, w_, h_, sf_, levels_, [synth.make_image(w_, h_, seed=190 + b) for b in range(9)])
    c_.close()
    print("cascade ok, repeat", 2 if "pyr" in os.environ.get("FT_DEBUG_REPEAT", "") else 1)

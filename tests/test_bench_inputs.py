"""The synthetic inputs of bench.py (CPU): every pair of a step is a distinct frame, shifted scenes stay rectified, the dense
mosaic scenes carry the candidate counts the second octree tier is for."""
import importlib.util
import os

import numpy as np

from fasttrack_amd import synth
from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod_inputs", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_stream_frames_are_distinct_and_rectified():
    bench = _bench()
    w, h, D, S = 160, 120, 12, 3
    hostL, hostR, base = bench.make_stream(lambda shape, dt: np.zeros(shape, dt), w, h, rank=1, D=D, scenes=S)
    assert hostL.shape == (D, h, w) and len(base) == S
    assert len({hostL[d].tobytes() for d in range(D)}) == D and len({hostR[d].tobytes() for d in range(D)}) == D
    for d in range(D):
        s, k = d % S, d // S
        dx, dy = (53 * k) % w, (29 * k) % h
        # the same cyclic shift for both images of a pair: rows stay aligned, disparities are kept
        assert np.array_equal(np.roll(hostL[d], (-dy, -dx), (0, 1)), base[s][0])
        assert np.array_equal(np.roll(hostR[d], (-dy, -dx), (0, 1)), base[s][1])
    other, _, _ = bench.make_stream(lambda shape, dt: np.zeros(shape, dt), w, h, rank=2, D=2, scenes=2)
    assert not np.array_equal(other[0], hostL[0])  # one stream per rank: different seeds


def test_mosaic_pair_is_dense_seeded_and_rectified():
    w, h = 320, 240
    L, R = synth.make_mosaic_pair(w, h, seed=4, block=8, disparity=12)
    L2, R2 = synth.make_mosaic_pair(w, h, seed=4, block=8, disparity=12)
    assert np.array_equal(L, L2) and np.array_equal(R, R2) and L.shape == (h, w) and L.dtype == np.uint8
    # right image = the same plane 12 px further left (up to the +-3 noise of each view)
    diff = np.abs(L[:, 12:].astype(int) - R[:, :-12].astype(int))
    assert diff.max() <= 6
    obj = synth.make_image(w, h, seed=4)
    exd, exo = ob.Extractor(500), ob.Extractor(500)
    exd.extract(L)
    exo.extract(obj)
    assert len(exd.candidates(0)) > 3 * len(exo.candidates(0))  # several times the FAST survivors of the object scenes


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """--dump-outputs on a batch too large to write whole: a fixed seeded sample of the pairs, at most 64 MB even with every
    image at the front end's keypoint capacity, the arrays of each sampled pair as the front end holds them"""
    from types import SimpleNamespace
    from fasttrack_amd import KP_DTYPE
    bench = _bench()
    B, cap = 300, 2100
    rng = np.random.default_rng(3)
    kL, kR = np.zeros((B, cap), KP_DTYPE), np.zeros((B, cap), KP_DTYPE)
    for k in (kL, kR):
        for f in ("x", "y", "size", "angle", "response"):
            k[f] = rng.random((B, cap), np.float32)
        k["octave"] = rng.integers(0, 8, (B, cap))
        k["class_id"] = -1
    fe = SimpleNamespace(capacity=cap, _kL=kL, _kR=kR, _dL=rng.integers(0, 256, (B, cap, 32), np.uint8),
                         _dR=rng.integers(0, 256, (B, cap, 32), np.uint8), _ur=rng.random((B, cap), np.float32),
                         _dp=rng.random((B, cap), np.float32), _nL=np.full(B, cap, np.int32), _nR=np.full(B, cap, np.int32),
                         _nm=rng.integers(0, cap, B).astype(np.int32))
    total = bench.dump_outputs(str(tmp_path / "a"), fe, B)
    bench.dump_outputs(str(tmp_path / "b"), fe, B)
    names = sorted(os.listdir(tmp_path / "a"))
    d = {n[:-4]: np.load(os.path.join(tmp_path, "a", n)) for n in names}
    assert total == sum(v.nbytes for v in d.values()) <= 64e6 and total > 48e6
    assert all(v.dtype in (np.float32, np.float64) for v in d.values())
    for n in names:
        assert np.array_equal(np.load(os.path.join(tmp_path, "a", n)), np.load(os.path.join(tmp_path, "b", n))), n
    pick = d["pairs"].astype(int)
    assert 1 < len(pick) < B and np.all(np.diff(pick) > 0) and pick[-1] < B
    assert np.array_equal(d["counts"], np.stack([fe._nL, fe._nR, fe._nm], -1))
    j = 1  # the second sampled pair
    b, rows = pick[j], slice(j * cap, (j + 1) * cap)
    assert np.array_equal(d["keys_left"][rows, 5], kL[b]["octave"]) and np.array_equal(d["keys_right"][rows, 0], kR[b]["x"])
    assert np.array_equal(d["desc_right"][rows], fe._dR[b]) and np.array_equal(d["uright"][rows], fe._ur[b])
    assert np.array_equal(d["depth"][rows], fe._dp[b]) and d["keys_left"].shape == (len(pick) * cap, 7)

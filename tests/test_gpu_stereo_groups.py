"""k_stereo_match in its workgroup-per-group form (needs an MI355X): 64 row-ordered left keypoints per workgroup, the
candidates of the group's rows staged in LDS in chunks of 256.  Inputs that bend the grouping - one bucket that holds every
right keypoint, all distances tied, rows at and off the image edges, left counts around the group size, bucket sizes around
the chunk size - against the oracle, bit for bit, and the idempotence the marginal-cost aid relies on."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fasttrack_amd import orb
from oracle import binding as ob
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, NF, SEED = 640, 480, 1000, 5
CHUNK = 256  # ST_CHUNK of kernels_stereo.hip


class _Rig:
    def __init__(self):
        self.ctx = orb.Context(0)
        self.fr = sc.oracle_stereo_frame(W, H, NF, SEED)
        self.exL = orb.ORBextractor(self.ctx, NF, 1.2, 8, 20, 7, W, H)
        self.exR = orb.ORBextractor(self.ctx, NF, 1.2, 8, 20, 7, W, H)
        self.exL(self.fr["L"])
        self.exR(self.fr["R"])

    def close(self):
        self.exL.close()
        self.exR.close()
        self.ctx.close()

    def check(self, kL, kR, dL, dR, expect_n=None, expect_cut_n=None):
        """both median-cut settings against the oracle; -> the oracle's result without the cut"""
        fr = self.fr
        mbf, mb = fr["intr"]["mbf"], fr["intr"]["mb"]
        first = None
        for cut in (False, True):
            o = ob.stereo_match(fr["exL"], fr["exR"], kL, kR, dL, dR, mbf, mb, median_cut=cut)
            g = orb.KernelController.launchStereoMatchKernel(self.exL, self.exR, kL, kR, dL, dR, mbf, mb, median_cut=cut)
            print(f"nL {len(kL)} nR {len(kR)} cut {cut}: oracle n {o['n']} gpu n {g['n']}")
            if not cut and expect_n is not None:
                assert o["n"] == expect_n
            if cut and expect_cut_n is not None:
                assert o["n"] == expect_cut_n
            assert g["n"] == o["n"]
            assert np.array_equal(g["uright"], o["uright"])
            assert np.array_equal(g["depth"], o["depth"])
            if not cut:
                assert np.array_equal(g["sad"], o["sad"])
                first = o
        return first


@pytest.fixture(scope="module")
def rig():
    r = _Rig()
    assert len(r.fr["kL"]) == 1008 and len(r.fr["kR"]) == 1004
    yield r
    r.close()


def _frac(y):
    return (y - np.floor(y)).astype(np.float32)


def test_base_frame(rig):
    fr = rig.fr
    o = rig.check(fr["kL"], fr["kR"], fr["dL"], fr["dR"])
    assert o["n"] > 20


def test_one_row(rig):
    """every keypoint in row 240: one bucket holds all 1 004 right keypoints and every group scans all of them (four chunks)"""
    fr = rig.fr
    kL, kR = fr["kL"].copy(), fr["kR"].copy()
    kL["y"] = np.float32(240) + _frac(kL["y"])
    kR["y"] = np.float32(240) + _frac(kR["y"])
    rig.check(kL, kR, fr["dL"], fr["dR"], expect_n=218)


def test_all_ties(rig):
    """every distance is 0: the lowest iR inside each lane's window must win whatever wave or chunk visits it"""
    fr = rig.fr
    dL, dR = np.repeat(fr["dL"][:1], len(fr["dL"]), 0), np.repeat(fr["dL"][:1], len(fr["dR"]), 0)
    rig.check(fr["kL"], fr["kR"], dL, dR, expect_n=415)


def test_rows_at_and_off_the_edges(rig):
    fr = rig.fr
    kL = fr["kL"].copy()
    kL["y"][:8] = np.array([-1, -0.5, 0, 0.5, H - 1, H - 0.5, H, H + 3], np.float32)
    o = rig.check(kL, fr["kR"], fr["dL"], fr["dR"], expect_n=223)
    assert (o["uright"][[0, 6, 7]] == -1).all() and (o["depth"][[0, 6, 7]] == -1).all()


@pytest.mark.parametrize("nL,n", [(1, 0), (63, 12), (64, 12), (65, 13), (129, 26)])
def test_ragged_left_counts(rig, nL, n):
    fr = rig.fr
    rig.check(fr["kL"][:nL], fr["kR"], fr["dL"][:nL], fr["dR"], expect_n=n)


@pytest.mark.parametrize("nR,n", [(1, 0), (63, 14), (65, 14)])
def test_few_right_keypoints(rig, nR, n):
    fr = rig.fr
    rig.check(fr["kL"], fr["kR"][:nR], fr["dL"], fr["dR"][:nR], expect_n=n)


@pytest.mark.parametrize("nR,n", [(127, 44), (128, 44), (129, 44), (257, 84), (CHUNK - 1, None), (CHUNK, None)])
def test_bucket_against_chunk_size(rig, nR, n):
    """two buckets' worth of right keypoints in rows every left keypoint reaches: the staged range is exactly nR entries"""
    fr = rig.fr
    kL, kR = fr["kL"].copy(), fr["kR"][:nR].copy()
    kR["y"] = np.float32(100) + np.float32(0.5) * (np.arange(nR) % 2).astype(np.float32)
    kL["y"] = np.float32(100.25)
    o = rig.check(kL, kR, fr["dL"], fr["dR"][:nR], expect_n=n)
    assert o["n"] > 0


REG_CAP = 64 * 40  # 64 * SM_PER_LANE of kernels_stereo.hip: the most left keypoints whose SADs k_stereo_median holds in registers


@pytest.mark.parametrize("nL,n,n_cut", [(REG_CAP, 582, 463), (REG_CAP + 1, 582, 463), (3024, 669, 540)])
def test_median_cut_in_registers_and_looped(rig, nL, n, n_cut):
    """k_stereo_median at and above its register capacity: the frame's left keypoints three times over, cut to the last count of
    the register path, the first of the path that re-reads the SADs in every bisection step, and all of them; the cut acts
    (the oracle drops a fifth of the matches)"""
    fr = rig.fr
    kL, dL = np.tile(fr["kL"], 3)[:nL], np.tile(fr["dL"], (3, 1))[:nL]
    assert len(kL) == nL and len(dL) == nL
    rig.check(kL, fr["kR"], dL, fr["dR"], expect_n=n, expect_cut_n=n_cut)


def test_idempotent_when_enqueued_twice():
    """FT_DEBUG_REPEAT is read once per process: a fresh child runs the base case with row sort and match enqueued twice"""
    env = dict(os.environ, FT_DEBUG_REPEAT="stereo,rowsort")
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_stereo_groups"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "base case ok, repeat 2" in r.stdout


if __name__ == "__main__":
    rig_ = _Rig()
    o_ = rig_.check(rig_.fr["kL"], rig_.fr["kR"], rig_.fr["dL"], rig_.fr["dR"])
    assert o_["n"] > 20
    rig_.close()
    print("base case ok, repeat", 2 if "stereo" in os.environ.get("FT_DEBUG_REPEAT", "") else 1)

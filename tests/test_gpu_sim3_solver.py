"""ft_sim3_solver on the device against the restatement of Sim3Solver (tests/sim3_solver_ref.py): every field of every result equal
- the integers, the flags and the per-iteration counts exactly, the floats bit for bit (the kernels evaluate the restatement's
text: the same Jacobi, glibc's sinf / cosf / atan2f written out, no contraction); independence from the batch, repeatability,
pinned inputs, problems without a job, invalid arguments."""
import ctypes as C

import numpy as np
import pytest

from fasttrack_amd import _capi, orb
from tests import sim3_solver_cases as sc

pytestmark = pytest.mark.gpu
INTS = ("converged", "no_more", "iterations", "effective_iterations", "n_inliers", "n_best_inliers", "best_iteration")
FLOATS = ("T12", "R", "t", "s")
ARRAYS = ("inliers", "best_inliers", "hypothesis_inliers")


@pytest.fixture(scope="module")
def ctx():
    c = orb.Context(0)
    yield c
    c.close()


def run(ctx, keys, pinned=None):
    return orb.sim3_solver(ctx, [sc.to_device(orb, sc.CASES[k], pinned=pinned) for k in keys])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differences(a, b):
    """the fields in which two results differ: integers and arrays by value, floats by their bits (a NaN equals itself)"""
    return [f for f in INTS if a[f] != b[f]] + [f for f in FLOATS if not np.array_equal(bits(a[f]), bits(b[f]))] + \
           [f for f in ARRAYS if not np.array_equal(a[f], b[f])]


@pytest.fixture(scope="module")
def all_cases(ctx):
    """every committed case in one call: 13 problems of every size, model pairing and ending, two of them without a job"""
    return dict(zip(sc.CASES, run(ctx, list(sc.CASES))))


@pytest.mark.parametrize("key", list(sc.CASES))
def test_case_is_the_restatement_bit_for_bit(all_cases, key):
    got, want = all_cases[key], sc.reference(key)
    assert differences(got, want) == [], (key, {f: (got[f], want[f]) for f in differences(got, want)})


@pytest.mark.parametrize("name", sorted(sc.BATCHES))
def test_batches_and_every_problem_alone(ctx, all_cases, name):
    keys = sc.BATCHES[name]
    got = run(ctx, keys)
    for k, g in zip(keys, got):
        assert differences(g, all_cases[k]) == [], k       # independent of what else is in the batch
        assert differences(run(ctx, [k])[0], g) == [], k  # and of being alone
    assert all(differences(a, b) == [] for a, b in zip(got, run(ctx, keys)))  # the same call twice


def test_pinned_inputs_give_the_same_bits(ctx, all_cases):
    keys = ["sparse_100_of_2000", "kb8_63_formula_142", "jobless_5", "n3_converges_first"]
    for k, g in zip(keys, run(ctx, keys, pinned=ctx)):
        assert differences(g, all_cases[k]) == [], k


def test_inliers_only_when_converged_and_never_without_a_pair(all_cases):
    for key, g in all_cases.items():
        P = sc.CASES[key]
        if not g["converged"]:
            assert not g["inliers"].any() and g["n_inliers"] == 0, key
        else:
            assert np.array_equal(g["inliers"], g["best_inliers"]) and g["n_inliers"] == g["inliers"].sum(), key
        assert not g["inliers"][P["valid"] == 0].any() and not g["best_inliers"][P["valid"] == 0].any(), key
        assert g["best_inliers"].sum() == g["n_best_inliers"], key


def test_jobless_problems_return_identity_without_a_launch(ctx):
    ctx.reset_stats()
    for g in run(ctx, sc.BATCHES["only_jobless"]):
        assert g["no_more"] and not g["converged"] and g["iterations"] == 0 and g["n_inliers"] == 0 and g["n_best_inliers"] == 0
        assert np.array_equal(g["T12"], np.eye(4, dtype=np.float32)) and np.array_equal(g["R"], np.eye(3, dtype=np.float32))
        assert g["s"] == 1 and not g["t"].any() and not g["inliers"].any() and not g["best_inliers"].any() and len(g["hypothesis_inliers"]) == 0
    assert ctx.get_stat("sim3_solver.launches")[1] == 0
    run(ctx, sc.BATCHES["jobless_in_the_middle"])
    run(ctx, sc.BATCHES["one"])
    assert ctx.get_stat("sim3_solver.launches") == (6.0, 2)  # three launches per call whatever it holds


def _call(ctx, problems, n=None):
    """a raw call with sentinel-filled outputs -> status, the outputs"""
    k = len(problems)
    Pa = (_capi.Sim3Problem * k)(*problems)
    R = (_capi.Sim3Result * k)()
    C.memset(R, 0x5a, C.sizeof(R))
    inl = [np.full(max(p.n, 1), 7, np.uint8) for p in problems]
    best = [np.full(max(p.n, 1), 7, np.uint8) for p in problems]
    hyp = [np.full(max(p.max_iterations, 1), -7, np.int32) for p in problems]
    arr = lambda v: (C.c_void_p * k)(*[_capi.ptr(a) for a in v])
    rc = _capi.lib().ft_sim3_solver(ctx._h, k if n is None else n, Pa, R, arr(inl), arr(best), arr(hyp))
    untouched = all((a == 7).all() for a in inl + best) and all((a == -7).all() for a in hyp) and bytes(R) == b"\x5a" * C.sizeof(R)
    return rc, untouched


def test_invalid_arguments_are_refused_without_a_launch(ctx):
    F = sc.CASES["mixed_64_two_fixscale"]
    ok = sc.to_device(orb, sc.CASES["n4_formula_35"])
    keep = []

    def variant(**change):
        d = sc.to_device(orb, F)
        keep.append(d)
        c = _capi.Sim3Problem.from_buffer_copy(d.c)
        for k, v in change.items():
            setattr(c, k, v)
        return c

    ctx.reset_stats()
    bad_q = variant()
    bad_q.Tcw2.q[3] = 2.0
    neg = np.array(F["rand_draws"], np.int32)
    neg[5] = -1  # behind the draws the two iterations read: every draw of 3 * max_iterations is checked
    few = np.zeros(64, np.uint8)
    few[:2] = 1  # two pairs, min_inliers 1: no sample of three
    cases = [variant(n=-1), variant(n=1 << 16), variant(valid=None), variant(world_pos1=None), variant(world_pos2=None), variant(sigma2_1=None),
             variant(sigma2_2=None), variant(rand_draws=None), variant(cam_model1=2), variant(cam_model2=-1), bad_q, variant(probability=0.0),
             variant(probability=1.0), variant(probability=float("nan")), variant(min_inliers=-1), variant(max_iterations=0),
             variant(rand_draws=_capi.ptr(neg)), variant(valid=_capi.ptr(few), min_inliers=1)]
    for i, c in enumerate(cases):
        rc, untouched = _call(ctx, [ok.c, c])  # behind a valid problem: nothing of it is written either
        assert rc == _capi.FT_ERR_INVALID and untouched, i
    assert _call(ctx, [ok.c], n=-1)[0] == _capi.FT_ERR_INVALID
    big = np.zeros(3 * (_capi.SIM3_MAX_ITERATIONS + 1), np.int32)
    rc, untouched = _call(ctx, [ok.c, variant(max_iterations=_capi.SIM3_MAX_ITERATIONS + 1, rand_draws=_capi.ptr(big))])
    assert rc == _capi.FT_ERR_CAPACITY and untouched
    assert ctx.get_stat("sim3_solver.launches")[1] == 0


def test_the_largest_iteration_count_runs(ctx):
    """max_iterations == FT_SIM3_MAX_ITERATIONS with a tiny epsilon: 1 024 effective iterations of 257 pairs, every count compared"""
    from tests import sim3_solver_ref as ref
    P = sc.problem(7, 257, 60, min_inliers=1, max_iterations=_capi.SIM3_MAX_ITERATIONS, scale=1.4, fill="out")
    g = orb.sim3_solver(ctx, [sc.to_device(orb, P)])[0]
    assert g["effective_iterations"] == _capi.SIM3_MAX_ITERATIONS == len(g["hypothesis_inliers"])
    assert differences(g, ref.sim3_solver(P)) == []

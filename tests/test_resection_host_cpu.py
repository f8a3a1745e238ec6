"""CPU: the host side of the spherical resection (csrc/sba_resection.hpp + csrc/sba_lm.hpp compiled with g++,
tests/harness/resection_harness.cpp) against the numpy restatements of tests/resection_reference.py: the layout of the reduce
pass's row, the DLT finish fed with long-double moments, the log map at the rotations where the frame changes, and the LM
schedule driven by a numpy evaluator.  Also the condition the GPU tests put on their scenes: plain float64 numpy, in its own
summation order, stays within REL_TOL_F64 of the long-double sums."""
import ctypes as C

import numpy as np
import pytest

import pose_edges
import resection_reference as rr
from helpers import REL_TOL_F64, RT_TOL_F64

_U = np.array([1.8, -1.9, 1.7]) / np.linalg.norm([1.8, -1.9, 1.7])
# noisy scenes of the DLT comparison: (n, seed), each with lambda_2 / lambda_12 >= 1e-5 in the numpy reference (asserted below;
# 2.9e-4 ... 4.7e-2 when they were chosen)
NOISY = [(7, 200), (7, 202), (65, 200), (65, 203), (513, 201)]
# LM scenes with 8 % planted outliers at delta = 0.02: (n, seed); the float64 and the long-double evaluator take the same steps
LM_SCENES = [(65, 300), (65, 301), (513, 300), (513, 303)]
LM_DELTA = 0.02


def test_row_layout_and_expansion():
    h = rr.harness()
    assert [h.resection_harness_layout(k) for k in range(7)] == [0, 21, 27, 28, 29, 30, 32]
    s = rr.make_scene(65, 11, noise=1e-3, outliers=rr.planted(65))
    rot, tran = rr.start_near(s, 11)
    ref = rr.sums(s.X, s.y, rot, tran, LM_DELTA)
    assert ref.n_outlier > 0
    row = rr.row_from_sums(ref)
    out = np.zeros(46)
    h.resection_harness_expand(rr._dp(row), rr._dp(out))
    assert np.array_equal(out[:36].reshape(6, 6), ref.H) and np.array_equal(out[36:42], ref.g)
    assert (out[42], out[43], out[44], out[45]) == (ref.cost, ref.sum_w, ref.n_outlier, ref.n_behind)
    # a row whose entries all differ: every slot lands where the layout says, H symmetric
    row = np.arange(1.0, 33.0)
    h.resection_harness_expand(rr._dp(row), rr._dp(out))
    H = out[:36].reshape(6, 6)
    assert np.array_equal(H, H.T) and np.array_equal(H[np.triu_indices(6)], row[:21])
    assert np.array_equal(out[36:], row[21:31])


def test_reference_jacobian_and_scale_invariance():
    """The restatement itself: P [A | I] is the derivative of r (central differences), r does not move when a bearing is scaled."""
    s = rr.make_scene(20, 1, noise=1e-3)
    rot, tran = rr.start_near(s, 1)
    _, _, r, J, _ = rr.per_match(s.X, s.y, rot, tran, np.float64)
    h = 1e-6
    for k in range(6):
        dp = np.zeros(6)
        dp[k] = h
        rp = rr.per_match(s.X, s.y, rot + dp[:3], tran + dp[3:], np.float64)[2]
        rm = rr.per_match(s.X, s.y, rot - dp[:3], tran - dp[3:], np.float64)[2]
        assert np.abs((rp - rm) / (2 * h) - J[:, :, k]).max() < 1e-8
    scale = np.linspace(0.5, 3.0, 20)[:, None]
    assert np.abs(rr.per_match(s.X, s.y * scale, rot, tran, np.float64)[2] - r).max() < 1e-14


@pytest.mark.parametrize("n", [6, 7, 65, 513])
@pytest.mark.parametrize("pose", ["random", "near_pi", "identity"])
def test_dlt_recovers_noise_free_scenes(n, pose):
    rot = {"random": None, "near_pi": 3.14 * _U, "identity": np.zeros(3)}[pose]
    s = rr.make_scene(n, 100 + n, rot=rot)
    rc, r, t, l1, l2, l12, sv, scale = rr.harness_dlt(rr.moments(s.X, s.y).astype(np.float64), n)
    assert rc == 0
    assert np.abs(r - s.rot).max() <= RT_TOL_F64 and np.abs(t - s.tran).max() <= RT_TOL_F64
    assert l1 <= 1e-12 * l12 < l2 and np.abs(sv - 1.0).max() < 1e-9


@pytest.mark.parametrize("n,seed", NOISY)
def test_dlt_equals_numpy_on_noisy_scenes(n, seed):
    s = rr.make_scene(n, seed, noise=1e-3)
    mom = rr.moments(s.X, s.y).astype(np.float64)
    ref = rr.dlt(mom)
    assert ref.lam[1] / ref.lam[11] >= 1e-5           # the seeds were chosen for this
    rc, r, t, l1, l2, l12, sv, scale = rr.harness_dlt(mom, n)
    assert rc == 0
    assert np.abs(r - ref.rot).max() <= RT_TOL_F64 and np.abs(t - ref.tran).max() <= RT_TOL_F64
    assert abs(l2 - ref.lam[1]) <= 1e-9 * ref.lam[11] and abs(l12 - ref.lam[11]) <= 1e-9 * ref.lam[11]
    assert np.abs(sv - ref.sv).max() <= 1e-9
    assert 1e-5 < np.abs(r - s.rot).max() < 1e-1      # noise moves the linear answer: a start, not a solution


def test_dlt_refusals():
    s = rr.make_scene(65, 5, planar=True)
    mom = rr.moments(s.X, s.y).astype(np.float64)
    assert np.linalg.eigvalsh(rr.expand_moments(mom))[3] < 1e-12 * mom.max()      # the four-dimensional null space
    rc, r, t, *_ = rr.harness_dlt(mom, 65)
    assert rc == -6 and np.isnan(r).all() and np.isnan(t).all()
    s = rr.make_scene(5, 5)
    assert rr.harness_dlt(rr.moments(s.X, s.y).astype(np.float64), 5)[0] == -6
    s = rr.make_scene(7, 5)
    mom = rr.moments(s.X, s.y).astype(np.float64)
    assert rr.harness_dlt(mom, 7)[0] == 0
    mom[17] = np.nan
    assert rr.harness_dlt(mom, 7)[0] == -6


@pytest.mark.parametrize("name", pose_edges.NAMES)
def test_log_map_round_trips_the_rotation(name):
    h = rr.harness()
    w = np.ascontiguousarray(pose_edges.POSES[name])
    R, back, R2 = np.zeros(9), np.zeros(3), np.zeros(9)
    h.resection_harness_rotation(rr._dp(w), rr._dp(R))
    h.resection_harness_log(rr._dp(R), rr._dp(back))
    h.resection_harness_rotation(rr._dp(back), rr._dp(R2))
    assert np.abs(R2 - R).max() <= 1e-15
    if np.linalg.norm(w) < np.pi:
        assert np.abs(back - w).max() <= 1e-15 * max(1.0, np.linalg.norm(w))
    else:                                              # past pi the vector of the same rotation with angle 2 pi - |w|
        th = np.linalg.norm(w)
        assert np.abs(back - w * (th - 2 * np.pi) / th).max() <= 1e-14
    assert np.abs(back - rr.log_map(R.reshape(3, 3))).max() <= 1e-14


@pytest.mark.parametrize("n,seed", LM_SCENES)
def test_lm_on_f32_rounded_inputs_takes_the_same_steps_in_either_precision(n, seed):
    """What the GPU test of f32 planes relies on: the same scenes with the inputs rounded to f32."""
    s = rr.make_scene(n, seed, noise=1e-3, outliers=rr.planted(n))
    X, y = rr.planes(s, True)
    rc, r0, t0, *_ = rr.harness_dlt(rr.moments(X, y).astype(np.float64), n)
    assert rc == 0
    _, _, sm, rc = rr.harness_solve(r0, t0, rr.numpy_evaluator(X, y, LM_DELTA))
    _, _, sl, rcl = rr.harness_solve(r0, t0, rr.numpy_evaluator(X, y, LM_DELTA, np.longdouble))
    assert rc == 0 and rcl == 0
    assert (sm.termination, sm.num_iterations, sm.num_successful_steps, sm.num_evaluations) == \
           (sl.termination, sl.num_iterations, sl.num_successful_steps, sl.num_evaluations)


@pytest.mark.parametrize("n", [63, 64, 65, 511, 512, 513, 1023, 1024, 1025])
def test_numpy_dlt_is_well_conditioned_on_the_gpu_scenes(n):
    """The noisy scenes on which the GPU test compares the guess with the numpy DLT: lambda_2 / lambda_12 >= 1e-5, f32-rounded too."""
    s = rr.make_scene(n, 500 + n, noise=1e-3)
    for f32 in (False, True):
        X, y = rr.planes(s, f32)
        lam = rr.dlt(rr.moments(X, y).astype(np.float64)).lam
        assert lam[1] / lam[11] >= 1e-5


@pytest.mark.parametrize("n,seed", LM_SCENES)
def test_lm_converges_from_the_dlt_start_with_outliers(n, seed):
    """Bearing noise 1e-3 at depths up to 10 moves a landmark's ray by up to 1e-2; over the ~0.92 n inliers the pose moves by
    about 1e-3 * 6 / sqrt(n): 7e-4 at n = 65.  Four times that bounds the distance to the truth."""
    s = rr.make_scene(n, seed, noise=1e-3, outliers=rr.planted(n))
    rc, r0, t0, *_ = rr.harness_dlt(rr.moments(s.X, s.y).astype(np.float64), n)
    assert rc == 0
    r, t, sm, rc = rr.harness_solve(r0, t0, rr.numpy_evaluator(s.X, s.y, LM_DELTA))
    rl, tl, sl, rcl = rr.harness_solve(r0, t0, rr.numpy_evaluator(s.X, s.y, LM_DELTA, np.longdouble))
    assert rc == 0 and rcl == 0
    assert sm.termination in (1, 2, 3)
    assert (sm.termination, sm.num_iterations, sm.num_successful_steps, sm.num_evaluations) == \
           (sl.termination, sl.num_iterations, sl.num_successful_steps, sl.num_evaluations)
    assert np.abs(r - rl).max() <= RT_TOL_F64 and np.abs(t - tl).max() <= RT_TOL_F64
    bound = 4 * 1e-3 * 6 / np.sqrt(65)
    assert np.abs(r - s.rot).max() <= bound and np.abs(t - s.tran).max() <= bound
    assert sm.final_cost < sm.initial_cost


def test_lm_limits():
    s = rr.make_scene(65, 300, noise=1e-3, outliers=rr.planted(65))
    r0, t0 = rr.start_near(s, 300)
    ev = rr.numpy_evaluator(s.X, s.y, LM_DELTA)
    r, t, sm, rc = rr.harness_solve(r0, t0, ev, max_num_iterations=1)
    assert rc == 0 and sm.termination == 4 and sm.num_iterations == 1 and sm.num_evaluations == 2
    r, t, sm, rc = rr.harness_solve(r0, t0, ev, tran_param=1)
    assert rc == 0 and abs(np.linalg.norm(t) - np.linalg.norm(t0)) <= 1e-14
    _, _, sm, rc = rr.harness_solve(r0, t0, lambda r_, t_: np.full(45, np.nan))
    assert rc != 0 and sm.termination == 6


EDGE_AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])


def edge_eval_scene(name):
    """Evaluated AT pose_edges.POSES[name] by the GPU tests: the truth is 3 degrees off, 8 % planted outliers."""
    return rr.make_scene(129, 62, noise=1e-3, outliers=rr.planted(129), rot=pose_edges.POSES[name] + np.deg2rad(3.0) * EDGE_AXIS)


def _float64_meets_the_bound(s, rot, tran, delta):
    ref, f64 = rr.sums(s.X, s.y, rot, tran, delta), rr.sums(s.X, s.y, rot, tran, delta, np.float64)
    sH = np.abs(ref.H).max()
    assert np.abs(f64.H - ref.H).max() <= REL_TOL_F64 * sH
    assert np.abs(f64.g - ref.g).max() <= 10 * REL_TOL_F64 * max(np.abs(ref.g).max(), REL_TOL_F64 * sH)
    assert abs(f64.cost - ref.cost) <= REL_TOL_F64 * ref.cost
    assert (f64.n_outlier, f64.n_behind, f64.sum_w > 0) == (ref.n_outlier, ref.n_behind, True)
    return ref


@pytest.mark.parametrize("name", pose_edges.NAMES)
def test_float64_numpy_meets_the_bound_at_the_pose_edges(name):
    s = edge_eval_scene(name)
    assert _float64_meets_the_bound(s, pose_edges.POSES[name], s.tran, LM_DELTA).n_outlier >= 1


# what the GPU tests evaluate at: sizes of f64 / f32 planes, (delta, planted outliers)
GPU_SIZES = (1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1537, 3073)
GPU_LOSSES = ((0.0, False), (0.02, True), (100.0, False))


@pytest.mark.parametrize("n", GPU_SIZES)
def test_float64_numpy_meets_the_bound_on_the_gpu_scenes(n):
    """The condition on the scenes of tests/test_gpu_resection.py: float64 in numpy's own order is within REL_TOL_F64 of long double."""
    for delta, with_outliers in GPU_LOSSES:
        s = rr.make_scene(n, 500 + n, noise=1e-3, outliers=rr.planted(n) if with_outliers else ())
        rot, tran = rr.start_near(s, n)
        ref = _float64_meets_the_bound(s, rot, tran, delta)
        if with_outliers and n >= 63:
            assert ref.n_outlier >= 1

"""CPU: the product's joint step logic (csrc/sba_joint_solver.hpp -- the state machine sba_problem_solve_joint runs between
device passes) driven by numpy-EMULATED passes, against the dense restatement tests/ref_joint_numpy.py.

The emulation (tests/joint_emulation.py) does what joint_reduce_kernel / joint_step_kernel do per match on the blocks
(e, w, E, F) of the restatement; the dense side never forms a Schur complement: it solves the whole (2n + m)-dim damped
system.  Both sides share JointProblem.blocks, so what is compared here is the elimination, the back-substitution and the
step logic -- not the Jacobian, whose independent check (explicit dR/dw against the kernels' J_l form) runs on the GPU.
"""
import numpy as np
import pytest

import ref_joint_numpy as rj
from helpers import RT_TOL_F64
from joint_emulation import EmulatedJoint, drive
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import synthetic


def scene(n, seed, sigma=1e-3, outliers=0.05, depth_noise=0.1):
    """full_rt scene with the start of the joint stage: perturbed pose, |t| at the true length (1), noisy depths."""
    return synthetic.full_rt(n, seed=seed, sigma=sigma, outlier_fraction=outliers, depth_noise=depth_noise)


@pytest.mark.parametrize("n", [8, 9, 257, 1000])
@pytest.mark.parametrize("outliers", [0.0, 0.1], ids=["clean", "huber_outliers"])
@pytest.mark.parametrize("tran_param", [cabi.TRAN_FREE, cabi.TRAN_SPHERE], ids=["free", "sphere"])
def test_one_step_schur_equals_dense(n, outliers, tran_param):
    """The Schur route's (delta d, delta c) is the dense solve's step.  Both routes are backward stable solves of the same
    damped system A, so each is within c * cond(A) * eps of the exact step relative to its norm; the bound used is
    16 * cond(A) * eps (c = 8 per route: Cholesky / LU growth of these small-bandwidth systems is O(1)), cond(A) computed
    (numpy.linalg.cond, 2-norm) at every input and printed."""
    cs = scene(n, seed=40 + n, outliers=outliers)
    for radius in (1e4, 1.0, 1e-2):
        opt = dict(rj.DEFAULTS, tran_param=tran_param, initial_trust_region_radius=radius)
        P = rj.JointProblem(cs.x1, cs.x2, 1.0)
        ref = rj.dense_step(P, cs.rot_init, cs.tran_init, cs.d12, radius, None, None, opt)
        assert ref["valid"]
        got = {}

        def on_step(r, em):
            got["delta_c"] = r[9:15].copy()
            got["delta_d"] = em.last_delta_d.copy()
        em = EmulatedJoint(cs.x1, cs.x2, cs.d12)
        drive(em, cs.rot_init, cs.tran_init, max_passes=2, on_step=on_step, tran_param=tran_param, initial_trust_region_radius=radius)
        full_ref = np.concatenate([ref["delta_d"].reshape(-1), ref["delta_c"]])
        full_got = np.concatenate([got["delta_d"].reshape(-1), got["delta_c"]])
        err = np.abs(full_got - full_ref).max() / np.abs(full_ref).max()
        tol = 16 * ref["cond"] * np.finfo(np.float64).eps
        print(f"n={n} outliers={outliers} tran_param={tran_param} radius={radius:g}: cond={ref['cond']:.3e} tol={tol:.3e} err={err:.3e}")
        assert err <= tol


SOLVE_CASES = [(200, 11, 0.0, 0.0), (200, 12, 1e-3, 0.0), (300, 13, 1e-3, 0.1), (64, 14, 2e-3, 0.1)]


@pytest.mark.parametrize("n,seed,sigma,outliers", SOLVE_CASES)
def test_whole_solve_matches_dense(n, seed, sigma, outliers):
    cs = scene(n, seed, sigma=sigma, outliers=outliers, depth_noise=0.05)
    rr, tr, dr, sr = rj.dense_solve(cs.x1, cs.x2, cs.rot_init, cs.tran_init, cs.d12)
    print(f"dense: {sr}")
    # no termination / acceptance test of the dense run sat within 1e-3 (relative) of its threshold: the counts are a fair yardstick
    assert sr["margin"] >= 1e-3, sr
    rot, tran, d, s, status, passes, _ = drive(EmulatedJoint(cs.x1, cs.x2, cs.d12), cs.rot_init, cs.tran_init)
    assert status == 0
    assert (rj.TERM[s.termination], s.num_iterations, s.num_successful_steps, s.num_evaluations) == \
        (sr["termination"], sr["num_iterations"], sr["num_successful_steps"], sr["num_evaluations"])
    assert passes == s.num_evaluations
    assert np.abs(rot - rr).max() <= RT_TOL_F64 and np.abs(tran - tr).max() <= RT_TOL_F64
    assert np.abs(d - dr).max() <= RT_TOL_F64 * np.abs(dr).max()
    assert abs(s.final_cost - sr["final_cost"]) <= 1e-9 * max(sr["final_cost"], 1e-30) + 1e-24
    assert abs(np.linalg.norm(tran) - np.linalg.norm(cs.tran_init)) <= 1e-12


def test_noise_free_known_answer():
    """From a pose a few degrees off and depths +-20 % off, |t| pinned at the true length, the planted rotation, translation
    and depths come back.  Tight tolerances (function = parameter = 0): the solve runs until the gradient tolerance or the
    iteration limit.  Reached: rot / tran within 1e-9, depths within 1e-8 relative (asserted below; the printed figures are
    smaller)."""
    n = 300
    cs = synthetic.full_rt(n, seed=21, sigma=0.0, outlier_fraction=0.0, perturb_deg=3.0)
    rng = np.random.default_rng(5)
    d0 = cs.d12 * rng.uniform(0.8, 1.2, size=cs.d12.shape)
    assert abs(np.linalg.norm(cs.tran_init) - np.linalg.norm(cs.tran_true)) < 1e-12
    rot, tran, d, s, status, _, _ = drive(EmulatedJoint(cs.x1, cs.x2, d0), cs.rot_init, cs.tran_init, function_tolerance=0.0,
                                          parameter_tolerance=0.0, max_num_iterations=100)
    print(f"known answer: {rj.TERM[s.termination]} after {s.num_iterations} iterations, cost {s.initial_cost:.3e} -> {s.final_cost:.3e}, "
          f"rot err {np.abs(rot - cs.rot_true).max():.2e}, tran err {np.abs(tran - cs.tran_true).max():.2e}, "
          f"depth rel err {(np.abs(d - cs.d12) / cs.d12).max():.2e}")
    assert status == 0
    assert np.abs(rot - cs.rot_true).max() <= 1e-9 and np.abs(tran - cs.tran_true).max() <= 1e-9
    assert (np.abs(d - cs.d12) / cs.d12).max() <= 1e-8


def test_free_translation_documents_the_gauge():
    """SBA_TRAN_FREE runs the functor as written: the cost is homogeneous in (d, t), so it falls monotonically and |t| shrinks."""
    cs = scene(200, 31, sigma=2e-3, outliers=0.0, depth_noise=0.05)
    rot, tran, d, s, status, _, trace = drive(EmulatedJoint(cs.x1, cs.x2, cs.d12), cs.rot_init, cs.tran_init, tran_param=cabi.TRAN_FREE)
    assert status == 0 and s.num_successful_steps >= 1
    costs = [c for c, _ in trace]
    assert all(b <= a for a, b in zip(costs, costs[1:])) and s.final_cost < s.initial_cost
    assert np.linalg.norm(tran) < np.linalg.norm(cs.tran_init)
    assert d.sum() < cs.d12.sum()


def test_limits_and_failures():
    cs = scene(50, 4)
    mk = lambda: EmulatedJoint(cs.x1, cs.x2, cs.d12)
    _, _, _, s, status, passes, _ = drive(mk(), cs.rot_init, cs.tran_init, max_num_iterations=0)
    assert rj.TERM[s.termination] == "no_convergence" and s.num_iterations == 0 and passes == 1
    _, _, _, s, status, passes, _ = drive(mk(), cs.rot_init, cs.tran_init, max_num_iterations=2)
    assert rj.TERM[s.termination] == "no_convergence" and s.num_iterations == 2
    _, _, _, s, status, passes, _ = drive(mk(), cs.rot_init, cs.tran_init, gradient_tolerance=1e30)
    assert rj.TERM[s.termination] == "gradient" and s.num_iterations == 0
    _, _, _, s, status, passes, _ = drive(mk(), cs.rot_init, cs.tran_init, initial_trust_region_radius=1e-40)
    assert rj.TERM[s.termination] == "min_radius"
    bad = mk()
    bad.d[0, 0] = np.nan
    d_before = bad.d.copy()
    _, _, d, s, status, passes, _ = drive(bad, cs.rot_init, cs.tran_init)
    assert rj.TERM[s.termination] == "failure" and status == cabi.SBA_ERR_NUMERIC and passes == 1
    assert np.array_equal(d, d_before, equal_nan=True)

"""CPU: the pass bound the batched joint solve's device loop relies on (csrc/sba_batch_joint.hip: batch_joint_solve_kernel runs at
most batch_joint_pass_bound(opt) = 2 * max_num_iterations + 2 trips).  The product's JointSolver (csrc/sba_joint_solver.hpp) is
driven over numpy-emulated passes (tests/joint_emulation.py); in feed_reduce every reduce pass either finishes the solve or
increments the iteration counter, and an iteration has at most one step pass -- so the number of passes of ANY run is at most
2 * max_num_iterations + 2, whichever way it terminates."""
import numpy as np
import pytest

from joint_emulation import EmulatedJoint, drive
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import synthetic


def _scene(n, seed, **kw):
    args = dict(sigma=1e-3, outlier_fraction=0.1, depth_noise=0.05)
    args.update(kw)
    return synthetic.full_rt(n, seed=synthetic.BASE_SEED + 170 + seed, **args)


def _run(c, **opt):
    rot, tran, d, s, status, passes, _ = drive(EmulatedJoint(c.x1, c.x2, c.d12), c.rot_init, c.tran_init, **opt)
    return s, status, passes


SCENES = [(300, 0, dict()), (200, 1, dict(sigma=0.0, outlier_fraction=0.0)), (257, 2, dict(sigma=2e-3)),
          (64, 3, dict(depth_noise=0.3)), (500, 4, dict(outlier_fraction=0.3))]


@pytest.mark.parametrize("n,seed,kw", SCENES)
@pytest.mark.parametrize("cap", [None, 0, 1, 2, 3, 7])
def test_passes_stay_within_the_bound(n, seed, kw, cap):
    c = _scene(n, seed, **kw)
    opt = {} if cap is None else dict(max_num_iterations=cap)
    s, status, passes = _run(c, **opt)
    its = 50 if cap is None else cap
    print(f"n={n} cap={cap}: {cabi.TERMINATION[s.termination]} after {s.num_iterations} iterations, {passes} passes (bound {2 * its + 2})")
    assert passes == s.num_evaluations
    assert passes <= 2 * its + 2
    assert s.num_iterations <= its


def test_a_small_cap_is_hit_and_reported():
    """A run that needs more iterations than the cap allows ends with NO_CONVERGENCE after exactly cap iterations: cap reduce
    passes that each start an iteration, cap step passes, and the reduce pass that meets the cap."""
    c = _scene(300, 0)
    free, _, _ = _run(c)
    assert free.num_iterations >= 4, free.num_iterations
    for cap in (1, 2, 3):
        s, status, passes = _run(c, max_num_iterations=cap)
        assert cabi.TERMINATION[s.termination] == "NO_CONVERGENCE" and status == 0
        assert s.num_iterations == cap and passes == 2 * cap + 1 <= 2 * cap + 2


def test_rejected_and_invalid_steps_count_as_iterations():
    """A tiny initial radius far from the minimum makes early steps short; a huge one on a noisy scene gets steps rejected.
    Either way every step pass belongs to an iteration of its own, so the bound holds with rejected steps in the run."""
    c = _scene(257, 2, sigma=2e-3)
    seen_rejected = False
    for radius in (1e-6, 1e4, 1e12):
        s, status, passes = _run(c, initial_trust_region_radius=radius, max_num_iterations=12)
        seen_rejected |= s.num_successful_steps < s.num_iterations - (1 if cabi.TERMINATION[s.termination].startswith("CONVERGENCE") else 0)
        assert passes <= 2 * 12 + 2 and s.num_iterations <= 12
    print("a run with rejected steps was among them:", seen_rejected)

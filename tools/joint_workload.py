#!/usr/bin/env python3
"""Workload for tools/profile_joint.sh: the joint solve (depths, rotation and translation together) next to the d-only
stage and the RT sweep, at 10^7 per-match-depth f64 matches.

    python tools/joint_workload.py [n] [iterations]

In ONE process (one box: boxes differ by ~6 %), on one handle:
  * 10 iterations of the d-only stage                      -> depth_step_kernel, the yardstick of the same run
  * 20 host-synchronous per-match RT sweeps                -> sweep_kernel, the other yardstick
  * two joint solves with zero tolerances (each runs to its fixed point or `iterations`: >= 20 LM iterations together)
                                                          -> joint_reduce_kernel, joint_step_kernel
  * end to end: staged pipeline (d-only, rot-only, tran-only) and then a joint refinement with default options, at n and
    at 2 048 matches (config C1; median of 20 runs)
Prints one JSON line with host-side wall times; the kernel times come from the rocprofv3 kernel trace."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from spherical_bundle_adjuster_amd import api, synthetic  # noqa: E402


def staged_then_joint(p, c, d0):
    """-> ms of the three stages, ms of the joint refinement, the joint summary"""
    p.set_depths(d0)
    t0 = time.perf_counter()
    d, _ = p.solve_depths(c.rot_init, c.tran_init)
    r1, t1, _ = p.solve(api.MODE_ROT, c.rot_init, c.tran_init, d[0, 0], d[1, 0])
    r2, t2, _ = p.solve(api.MODE_TRAN, r1, t1, d[0, 0], d[1, 0])
    t_staged = time.perf_counter()
    _, _, _, s = p.solve_joint(r2, t2, return_depths=False)
    t_joint = time.perf_counter()
    return 1e3 * (t_staged - t0), 1e3 * (t_joint - t_staged), s


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    out = {"n": n}
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 2, depth_noise=0.02)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        _, sd = p.solve_depths(c.rot_init, c.tran_init, options=api.default_lm_options(max_num_iterations=10))
        out["depth_stage"] = {"passes": sd.num_evaluations, "ms": 1e3 * sd.seconds_total}
        p.set_depths(c.d12)
        _, sec = p.eval_steps(api.MODE_RT, c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH, steps=20)
        out["rt_sweep_host_us_per_step"] = 1e6 * sec / 20
        opt = api.default_lm_options(tran_param=api.TRAN_SPHERE, function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0,
                                     max_num_iterations=iters)
        fixed = []
        for _ in range(2):        # a solve reaches its fixed point (cost change exactly 0) after ~18 iterations: two of them
            p.set_depths(c.d12)
            _, _, _, s = p.solve_joint(c.rot_init, c.tran_init, options=opt, return_depths=False)
            fixed.append(s)
        its, passes = sum(s.num_iterations for s in fixed), sum(s.num_evaluations for s in fixed)
        out["joint_fixed"] = {"iterations": its, "passes": passes, "termination": s.termination,
                              "ms": 1e3 * sum(s.seconds_total for s in fixed),
                              "host_us_per_iteration": 1e6 * sum(s.seconds_total for s in fixed) / max(its, 1),
                              "host_us_per_pass": 1e6 * sum(s.seconds_eval for s in fixed) / max(passes, 1),
                              "cost": [s.initial_cost, s.final_cost]}
        ms_staged, ms_joint, sj = staged_then_joint(p, c, np.full((n, 2), 6.0))
        out["end_to_end"] = {"staged_ms": ms_staged, "joint_ms": ms_joint, "joint_iterations": sj.num_iterations,
                             "joint_passes": sj.num_evaluations, "termination": sj.termination, "cost": [sj.initial_cost, sj.final_cost]}
    c1 = synthetic.full_rt(2048, seed=synthetic.BASE_SEED, sigma=2e-4, outlier_fraction=0.02)
    with api.Problem(0) as p:
        p.upload(c1.x1, c1.x2, np.full((2048, 2), 6.0))
        runs = [staged_then_joint(p, c1, np.full((2048, 2), 6.0)) for _ in range(21)][1:]
        out["c1_2048"] = {"staged_ms_median": float(np.median([r[0] for r in runs])), "joint_ms_median": float(np.median([r[1] for r in runs])),
                          "joint_iterations": runs[-1][2].num_iterations, "joint_passes": runs[-1][2].num_evaluations,
                          "termination": runs[-1][2].termination, "cost": [runs[-1][2].initial_cost, runs[-1][2].final_cost]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

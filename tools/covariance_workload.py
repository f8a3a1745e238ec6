#!/usr/bin/env python3
"""Workload for tools/profile_covariance.sh: the joint covariance next to the joint solve's reduce pass and the d-only stage,
at 10^7 per-match-depth f64 matches.

    python tools/covariance_workload.py [n] [calls]

In ONE process (one box: boxes differ by ~6 %), on one handle:
  * 10 iterations of the d-only stage                      -> depth_step_kernel, a yardstick of the same run
  * `calls` reduce passes of the joint solve (eval_joint)  -> joint_reduce_kernel, the other yardstick
  * `calls` covariance calls with the per-match blocks     -> cov_reduce_kernel, cov_depth_kernel
  * `calls` covariance calls without them (host wall time of the pose block alone)
Prints one JSON line with host-side wall times; the kernel times come from the rocprofv3 kernel trace."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from spherical_bundle_adjuster_amd import api, synthetic  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out = {"n": n, "calls": calls}
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 2, depth_noise=0.02)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        _, sd = p.solve_depths(c.rot_init, c.tran_init, options=api.default_lm_options(max_num_iterations=10))
        out["depth_stage"] = {"passes": sd.num_evaluations, "ms": 1e3 * sd.seconds_total}
        p.set_depths(c.d12)
        t0 = time.perf_counter()
        for _ in range(calls):
            eq = p.eval_joint(c.rot_init, c.tran_init)
        out["eval_joint_host_us"] = 1e6 * (time.perf_counter() - t0) / calls
        t0 = time.perf_counter()
        for _ in range(calls):
            pose = p.covariance_joint(c.rot_init, c.tran_init, depths=False)
        out["covariance_pose_host_us"] = 1e6 * (time.perf_counter() - t0) / calls
        t0 = time.perf_counter()
        for _ in range(calls):
            full = p.covariance_joint(c.rot_init, c.tran_init)
        out["covariance_full_host_us"] = 1e6 * (time.perf_counter() - t0) / calls      # includes the 24 B / match copy to the host
        assert full.cov.tobytes() == pose.cov.tobytes() and full.cost == pose.cost
        sd6 = np.sqrt(full.sigma2 * np.diag(full.cov))
        out["result"] = {"n_used": full.n_used, "n_degenerate": full.n_degenerate, "dim": full.dim, "cost": full.cost,
                         "eval_joint_cost": eq.cost, "sigma_rot_deg": list(np.rad2deg(sd6[:3])), "sigma_tran": list(sd6[3:]),
                         "median_sigma_d1": float(np.sqrt(full.sigma2 * np.median(full.depth_cov[:, 0])))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Workload for tools/profile_structure.sh: the triangulated structure next to the joint covariance's depth pass and the d-only
stage, at 10^7 per-match-depth f64 matches.

    python tools/structure_workload.py [n] [calls]

In ONE process (one box: boxes differ by ~6 %), on one handle:
  * 10 iterations of the d-only stage                                   -> depth_step_kernel, a yardstick of the same run
  * `calls` covariance calls with the per-match blocks copied to the host -> cov_depth_kernel, the other yardstick, and the
                                                                           host wall time the device form is set against
  * `calls` structure_joint_into calls, all three outputs into torch tensors -> structure_kernel<.., true, true, true>
  * `calls` structure_joint_into calls, the score alone                    -> structure_kernel<.., false, false, true>
  * `calls` structure_order_stats calls (score-only pass + selection)
  * 3 structure_joint calls, all outputs copied to the host (80 B / match over PCIe into pageable memory)
Prints one JSON line with host-side wall times; the kernel times come from the rocprofv3 kernel trace."""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from spherical_bundle_adjuster_amd import api, synthetic  # noqa: E402


def timed(calls, f):
    t0 = time.perf_counter()
    for _ in range(calls):
        r = f()
    return 1e6 * (time.perf_counter() - t0) / calls, r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out = {"n": n, "calls": calls}
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 2, depth_noise=0.02)
    rot, tran = c.rot_init, c.tran_init
    dev = torch.device("cuda", 0)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        _, sd = p.solve_depths(rot, tran, options=api.default_lm_options(max_num_iterations=10))
        out["depth_stage"] = {"passes": sd.num_evaluations, "ms": 1e3 * sd.seconds_total}
        p.set_depths(c.d12)
        out["covariance_pose_host_us"], pose = timed(calls, lambda: p.covariance_joint(rot, tran, depths=False))
        out["covariance_full_host_us"], full = timed(calls, lambda: p.covariance_joint(rot, tran))     # 24 B / match to the host
        xyz = torch.empty((n, 3), dtype=torch.float64, device=dev)
        cov = torch.empty((n, 6), dtype=torch.float64, device=dev)
        score = torch.empty((n,), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        p.structure_joint_into(xyz.data_ptr(), cov.data_ptr(), score.data_ptr(), rot, tran)          # first call: occupancy query
        out["structure_into_all_host_us"], into = timed(calls, lambda: p.structure_joint_into(xyz.data_ptr(), cov.data_ptr(), score.data_ptr(), rot, tran))
        out["structure_into_score_host_us"], _ = timed(calls, lambda: p.structure_joint_into(None, None, score.data_ptr(), rot, tran))
        k = api.quantile_rank([0.5, 0.9], n)
        out["structure_order_stats_host_us"], q = timed(calls, lambda: p.structure_order_stats(rot, tran, k))
        out["structure_host_form_host_us"], host = timed(3, lambda: p.structure_joint(rot, tran))
        assert into.cov.tobytes() == pose.cov.tobytes() == full.cov.tobytes() == host.pose.cov.tobytes()
        s = score.cpu().numpy()
        assert s.tobytes() == host.score.tobytes() and xyz.cpu().numpy().tobytes() == host.xyz.tobytes()
        assert q.tobytes() == np.partition(s, k)[k].tobytes()
        out["result"] = {"n_used": full.n_used, "n_degenerate": full.n_degenerate, "dim": full.dim, "sigma2": full.sigma2,
                         "score_median_scaled": float(full.sigma2 * q[0]), "score_p90_scaled": float(full.sigma2 * q[1]),
                         "median_sigma_x": float(np.sqrt(full.sigma2 * np.median(host.cov[:, 0])))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Workload for tools/profile_resection_consensus.sh: the robust resection guess at 10^7 per-match-depth f64 matches.

    python tools/resection_consensus_workload.py [n] [calls]

In ONE process (one box: boxes differ by ~6 %), on one handle holding a full_rt scene (landmarks d1 * x1, bearings x2, 5 % wrong
matches, bearing noise 1e-3):
  * `calls` score_resection calls with 128 candidates and `calls` with 1024 -> resect_score_kernel<double>
  * 3 resection_guess calls                                                 -> resect_moments_kernel, the refit pass's yardstick
  * 3 resection_guess_consensus calls (128 trials of 6, refit)              -> gather, score (128 + 1), inlier moments, reduce
  * one solve_resection from the consensus guess
Prints one JSON line with host-side wall times; the kernel times come from the rocprofv3 kernel trace."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from spherical_bundle_adjuster_amd import api, synthetic  # noqa: E402

THRESHOLD = 0.1     # bearing noise 1e-3 at depths up to 20 moves a landmark's ray by 2e-2 and a few times that in the tail


def timed(calls, f):
    t0 = time.perf_counter()
    for _ in range(calls):
        r = f()
    return 1e6 * (time.perf_counter() - t0) / calls, r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out = {"n": n, "calls": calls, "threshold": THRESHOLD}
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 3)
    rng = np.random.default_rng(11)
    step = 10.0 ** rng.uniform(-4.0, 0.0, size=(1024, 1))
    rots = c.rot_true + step * rng.standard_normal((1024, 3))
    trans = c.tran_true + step * rng.standard_normal((1024, 3))
    rots[0], trans[0] = c.rot_true, c.tran_true
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        p.score_resection(rots[:2], trans[:2], THRESHOLD)                           # first call: work memory
        out["score_128_host_us"], s128 = timed(calls, lambda: p.score_resection(rots[:128], trans[:128], THRESHOLD))
        out["score_1024_host_us"], s1024 = timed(calls, lambda: p.score_resection(rots, trans, THRESHOLD))
        out["resection_guess_host_us"], plain = timed(3, lambda: p.resection_guess())
        out["consensus_host_us"], g = timed(3, lambda: p.resection_guess_consensus(THRESHOLD, trials=128, seed=7))
        t0 = time.perf_counter()
        r, t, sm, nb = p.solve_resection(g.rot, g.tran, api.default_lm_options(huber_delta=THRESHOLD), store_depths=False)
        out["solve_resection"] = {"ms": 1e3 * (time.perf_counter() - t0), "termination": sm.termination, "evaluations": sm.num_evaluations,
                                  "rot_err": float(np.abs(r - c.rot_true).max()), "tran_err": float(np.abs(t - c.tran_true).max())}
        out["result"] = {"inliers_at_truth": int(s1024[0]), "score_min": int(s1024.min()), "score_max": int(s1024.max()),
                         "prefix_equal": bool(np.array_equal(s128, s1024[:128])), "consensus_inliers": g.n_inlier,
                         "best_trial_inliers": g.best_trial_inliers, "refit_used": g.refit_used, "valid_trials": g.n_valid_trials,
                         "consensus_rot_err": float(np.abs(g.rot - c.rot_true).max()),
                         "plain_guess_rot_err": float(np.abs(plain.rot - c.rot_true).max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Workload for tools/profile_resection_weighted.sh: the passes of the covariance-weighted resection next to the unweighted
reduce pass, at 10^7 per-match-depth f64 matches.

    python tools/resection_weighted_workload.py [n] [calls]

In ONE process (one box: boxes differ by ~6 %), on one handle holding a full_rt scene (landmarks d1 * x1, bearings x2) with a
seeded covariance per landmark (sigma_t = 0.002 |X| U(0.5, 2) across the viewing ray, sigma_r / sigma_t log-uniform in [3, 100]):
  * `calls` eval_resection calls with the loss and `calls` without    -> resect_reduce_kernel<double, *>: the BASELINE of the run
  * 3 freeze_resection_weights calls                                  -> resect_weights_kernel
  * `calls` eval_resection_weighted calls with the loss, then without -> resect_wreduce_kernel<double, *>
  * one resection_weights call                                        -> resect_weight_rows_kernel
  * one solve_resection, one solve_resection_weighted (2 rounds) from its result and one resection_covariance
Prints one JSON line with host-side wall times; the kernel times come from the rocprofv3 kernel trace."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from spherical_bundle_adjuster_amd import api, synthetic  # noqa: E402


def timed(calls, f):
    t0 = time.perf_counter()
    for _ in range(calls):
        r = f()
    return 1e6 * (time.perf_counter() - t0) / calls, r


def covariances(X, seed):
    """(n, 6) rows (xx, yy, zz, xy, xz, yz), built column by column to keep the peak memory at a few planes."""
    rng = np.random.default_rng(seed)
    n = len(X)
    norm = np.linalg.norm(X, axis=1)
    st2 = (0.002 * norm * rng.uniform(0.5, 2.0, size=n)) ** 2
    sr2 = st2 * np.exp(rng.uniform(np.log(3.0), np.log(100.0), size=n)) ** 2
    u = X / norm[:, None]
    rows = np.empty((n, 6))
    for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        rows[:, k] = (sr2 - st2) * u[:, a] * u[:, b] + (st2 if a == b else 0.0)
    return rows


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out = {"n": n, "calls": calls}
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 3)
    rot, tran = c.rot_init, c.tran_init
    cov = covariances(c.x1 * c.d12[:, :1], synthetic.BASE_SEED + 4)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        loss, plain = api.default_lm_options(huber_delta=2.0), api.default_lm_options(huber_delta=0.0)
        p.eval_resection(rot, tran, loss)                                          # first call: occupancy query
        out["eval_resection_loss_host_us"], _ = timed(calls, lambda: p.eval_resection(rot, tran, loss))
        out["eval_resection_plain_host_us"], _ = timed(calls, lambda: p.eval_resection(rot, tran, plain))
        t0 = time.perf_counter()
        p.set_landmark_covariances(cov)
        out["set_landmark_covariances_ms"] = 1e3 * (time.perf_counter() - t0)
        out["freeze_host_us"], nz = timed(3, lambda: p.freeze_resection_weights(rot, tran, 1e-3))
        p.eval_resection_weighted(rot, tran, loss)
        out["eval_weighted_loss_host_us"], eq = timed(calls, lambda: p.eval_resection_weighted(rot, tran, loss))
        out["eval_weighted_plain_host_us"], _ = timed(calls, lambda: p.eval_resection_weighted(rot, tran, plain))
        t0 = time.perf_counter()
        rows = p.resection_weights()
        out["resection_weights_ms"] = 1e3 * (time.perf_counter() - t0)
        # the pipeline a caller runs: the unweighted solve, then two weighted rounds from its result
        r, t, _, _ = p.solve_resection(rot, tran, api.default_lm_options(huber_delta=1.0), store_depths=False)
        t0 = time.perf_counter()
        r, t, sm, nb = p.solve_resection_weighted(r, t, loss, bearing_sigma=1e-3, reweight_rounds=2, store_depths=False)
        out["solve_weighted"] = {"ms": 1e3 * (time.perf_counter() - t0), "termination": sm.termination, "evaluations": sm.num_evaluations,
                                 "rot_err": float(np.abs(r - c.rot_true).max()), "tran_err": float(np.abs(t - c.tran_true).max()),
                                 "n_behind": nb}
        cv = p.resection_covariance(r, t, loss)
        out["result"] = {"cost": eq.cost, "n_outlier": eq.n_outlier, "n_behind": eq.n_behind, "n_zero_weight": nz,
                         "rows_finite": bool(np.isfinite(rows).all()), "sigma2": cv.sigma2, "dof": cv.dof,
                         "sigma_rot": float(np.sqrt(np.trace(cv.cov[:3, :3]))), "sigma_tran": float(np.sqrt(np.trace(cv.cov[3:, 3:])))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Config C5 (256 pairs x 50 000 matches, per-match f64) through the batched joint covariance, and the route it replaces.

    python tools/batch_covariance_workload.py [--pairs 256] [--matches 50000] [--repeat 5]

In ONE process (one box, the same data), on one batch:
  * `repeat` Batch.covariance_joint calls with the per-match blocks     -> batch_cov_kernel with the depth phase, the copy back
  * `repeat` calls with depths=False                                     -> batch_cov_kernel, reduce + finish only
  * the same two under the lock-step driver (SBA_BATCH_DEVICE_COV=0), outputs compared to the bit
  * the route a user had before: one Problem.upload + Problem.covariance_joint per pair, with and without the blocks
Prints one JSON line per measurement (host wall times); the kernel times come from the rocprofv3 kernel trace of
tools/profile_batch_covariance.sh."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spherical_bundle_adjuster_amd import api, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--matches", type=int, default=50_000)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    B, n = a.pairs, a.matches
    c = synthetic.full_rt(B * n, seed=synthetic.BASE_SEED + 5, depth_noise=0.02)
    off = (np.arange(B + 1) * n).astype(np.uint64)
    rot0 = np.tile(c.rot_init, (B, 1)); tran0 = np.tile(c.tran_init, (B, 1))

    results = {}
    for driver in ("device", "lock-step"):
        if driver == "lock-step":
            os.environ["SBA_BATCH_DEVICE_COV"] = "0"
        else:
            os.environ.pop("SBA_BATCH_DEVICE_COV", None)
        with api.Batch(0) as b:
            b.upload(c.x1, c.x2, off, c.d12)
            b.covariance_joint(rot0, tran0)              # allocations
            for depths in (True, False):
                times = []
                for _ in range(a.repeat):
                    t0 = time.perf_counter()
                    r = b.covariance_joint(rot0, tran0, depths=depths)
                    times.append(time.perf_counter() - t0)
                results[driver, depths] = r
                print(json.dumps({"what": f"Batch.covariance_joint {B} x {n}, driver {driver}, depths={depths}",
                                  "ms_median": statistics.median(times) * 1e3, "ms_all": [t * 1e3 for t in times],
                                  "failed_pairs": int(np.count_nonzero(r.status)), "n_used": int(r.n_used.sum()),
                                  "n_degenerate": int(r.n_degenerate.sum())}), flush=True)
    os.environ.pop("SBA_BATCH_DEVICE_COV", None)
    same = all(getattr(results["device", d], k).tobytes() == getattr(results["lock-step", d], k).tobytes()
               for d in (True, False) for k in ("cov", "cost", "sum_w", "n_used", "n_degenerate", "dim", "dof", "status"))
    same = same and results["device", True].depth_cov.tobytes() == results["lock-step", True].depth_cov.tobytes()
    print(json.dumps({"what": "drivers agree to the bit", "value": bool(same)}), flush=True)

    full = results["device", True]
    for depths in (True, False):
        times, worst = [], 0.0
        for _ in range(max(1, a.repeat // 2)):
            t0 = time.perf_counter()
            with api.Problem(0) as p:
                for g in range(B):
                    lo, hi = g * n, (g + 1) * n
                    p.upload(c.x1[lo:hi], c.x2[lo:hi], c.d12[lo:hi])
                    one = p.covariance_joint(c.rot_init, c.tran_init, depths=depths)
                    if g % 64 == 0:
                        worst = max(worst, float(np.abs(one.cov - full.cov[g]).max() / np.abs(one.cov).max()))
            times.append(time.perf_counter() - t0)
        print(json.dumps({"what": f"{B} x (Problem.upload + Problem.covariance_joint) at {n} matches, depths={depths}",
                          "ms_median": statistics.median(times) * 1e3, "ms_all": [t * 1e3 for t in times],
                          "max_rel_cov_difference_to_batch": worst}), flush=True)


if __name__ == "__main__":
    main()

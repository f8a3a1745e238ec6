#!/usr/bin/env python3
"""Config C5 (256 pairs x 50 000 matches, per-match f64) through the batched joint solve, and the yardstick it replaces.

  --mode batch     Batch.solve_joint: wall clock of the call (median of --repeat), depths staying on the device
  --mode lockstep  the same with SBA_BATCH_DEVICE_JOINT=0: one batch_joint_pass_kernel launch per pass -- the form to run under
                   `rocprofv3 --kernel-trace --stats` for the per-pass device time (reduce and step passes alternate; the
                   lock-step run prints how many launches of either kind it made, and the pair-passes that took part)
  --mode single    what a user did before: one Problem.upload + Problem.solve_joint per pair on the same pairs, wall clock
  --mode all       batch, lockstep, single in one process (same box, same data)
  --single-n N     also one Problem.solve_joint at N matches (the single-problem kernels' figures in the same run)

Prints one JSON line per measurement."""
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
    ap.add_argument("--mode", default="all", choices=("batch", "lockstep", "single", "all"))
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--matches", type=int, default=50_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--single-n", type=int, default=0)
    a = ap.parse_args()
    B, n = a.pairs, a.matches
    c = synthetic.full_rt(B * n, seed=synthetic.BASE_SEED + 5, depth_noise=0.02)
    off = (np.arange(B + 1) * n).astype(np.uint64)
    rot0 = np.tile(c.rot_init, (B, 1)); tran0 = np.tile(c.tran_init, (B, 1))
    modes = ("batch", "lockstep", "single") if a.mode == "all" else (a.mode,)

    for mode in modes:
        if mode == "single":
            times = []
            for _ in range(max(1, a.repeat // 2)):
                t0 = time.perf_counter()
                its = 0
                with api.Problem(0) as p:
                    for g in range(B):
                        lo, hi = g * n, (g + 1) * n
                        p.upload(c.x1[lo:hi], c.x2[lo:hi], c.d12[lo:hi])
                        _, _, _, s = p.solve_joint(c.rot_init, c.tran_init, return_depths=False)
                        its += s.num_evaluations
                times.append(time.perf_counter() - t0)
            print(json.dumps({"what": f"{B} x (Problem.upload + Problem.solve_joint) at {n} matches", "ms_median": statistics.median(times) * 1e3,
                              "ms_all": [t * 1e3 for t in times], "passes_total": its}), flush=True)
            continue
        if mode == "lockstep":
            os.environ["SBA_BATCH_DEVICE_JOINT"] = "0"
        else:
            os.environ.pop("SBA_BATCH_DEVICE_JOINT", None)
        with api.Batch(0) as b:
            t0 = time.perf_counter()
            b.upload(c.x1, c.x2, off, c.d12)
            upload_ms = (time.perf_counter() - t0) * 1e3
            b.solve_joint(rot0, tran0, return_depths=False)              # allocations
            times = []
            for _ in range(a.repeat):
                b.set_depths(c.d12)
                t0 = time.perf_counter()
                rot, tran, _, sums, status = b.solve_joint(rot0, tran0, return_depths=False)
                times.append(time.perf_counter() - t0)
            ev = [s.num_evaluations for s in sums]
            # every reduce pass either ends the solve or starts an iteration: a solve that ends in a step pass (function /
            # parameter tolerance) ran num_iterations reduce passes, any other num_iterations + 1; the rest were step passes
            reduce_passes = [s.num_iterations + (0 if s.termination in ("CONVERGENCE_FUNCTION", "CONVERGENCE_PARAMETER") else 1) for s in sums]
            print(json.dumps({"what": f"Batch.solve_joint {B} x {n}, driver {'lock-step' if mode == 'lockstep' else 'device'}",
                              "ms_median": statistics.median(times) * 1e3, "ms_all": [t * 1e3 for t in times], "upload_ms": upload_ms,
                              "failed_pairs": int(np.count_nonzero(status)), "passes_per_pair_min_max": [min(ev), max(ev)],
                              "pair_passes_total": sum(ev), "pair_reduce_passes": sum(reduce_passes), "pair_step_passes": sum(ev) - sum(reduce_passes),
                              "launches_lock_step": max(ev), "final_cost_sum": float(sum(s.final_cost for s in sums))}), flush=True)
    os.environ.pop("SBA_BATCH_DEVICE_JOINT", None)
    if a.single_n > 0:
        cs = synthetic.full_rt(a.single_n, depth_noise=0.02)
        with api.Problem(0) as p:
            p.upload(cs.x1, cs.x2, cs.d12)
            t0 = time.perf_counter()
            _, _, _, s = p.solve_joint(cs.rot_init, cs.tran_init, return_depths=False)
            print(json.dumps({"what": f"Problem.solve_joint at {a.single_n} matches", "ms": (time.perf_counter() - t0) * 1e3,
                              "passes": s.num_evaluations, "iterations": s.num_iterations}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Config C5 (256 pairs x 50 000 matches, per-match f64) through the batched structure, and the routes it replaces.

    python tools/batch_structure_workload.py [--pairs 256] [--matches 50000] [--repeat 5]

In ONE process (one box, the same data):
  * `repeat` Batch.structure_joint_into calls, all three outputs into device tensors  -> batch_cov_kernel (reduce + finish)
                                                                                         + batch_structure_kernel<all outputs>
  * `repeat` Batch.structure_joint_into calls, the score alone                        -> ... + batch_structure_kernel<score>
  * `repeat` Batch.structure_joint calls (host form: 80 B per match cross to the host)
  * `repeat` Batch.covariance_joint calls with the per-match depth rows (the host-copy route of DESIGN.md section 3.14)
  * Batch.structure_keep_below(0.5, 4.0) on a fresh upload each time (the upload is not timed)
  * the route a user had before: one Problem.upload + Problem.structure_joint_into per pair
Prints one JSON line per measurement (host wall times); the kernel times come from the rocprofv3 kernel trace of
tools/profile_batch_structure.sh."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spherical_bundle_adjuster_amd import api, synthetic  # noqa: E402


def timed(fn, repeat):
    times, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, {"ms_median": statistics.median(times) * 1e3, "ms_all": [t * 1e3 for t in times]}


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
    dev = torch.device("cuda", 0)
    tx = torch.empty((B * n, 3), dtype=torch.float64, device=dev)
    tc = torch.empty((B * n, 6), dtype=torch.float64, device=dev)
    ts = torch.empty((B * n,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    say = lambda what, **kw: print(json.dumps({"what": what, **kw}), flush=True)

    with api.Batch(0) as b:
        b.upload(c.x1, c.x2, off, c.d12)
        b.structure_joint_into(tx.data_ptr(), tc.data_ptr(), ts.data_ptr(), rot0, tran0)        # allocations
        pose, t = timed(lambda: b.structure_joint_into(tx.data_ptr(), tc.data_ptr(), ts.data_ptr(), rot0, tran0), a.repeat)
        say(f"Batch.structure_joint_into {B} x {n}, all outputs", **t, failed_pairs=int(np.count_nonzero(pose.status)),
            n_used=int(pose.n_used.sum()), n_degenerate=int(pose.n_degenerate.sum()))
        _, t = timed(lambda: b.structure_joint_into(None, None, ts.data_ptr(), rot0, tran0), a.repeat)
        say(f"Batch.structure_joint_into {B} x {n}, score only", **t)
        b.structure_joint(rot0, tran0)                                                              # the staging scratch
        host, t = timed(lambda: b.structure_joint(rot0, tran0), a.repeat)
        say(f"Batch.structure_joint {B} x {n} (host form, all outputs)", **t)
        same = (tx.cpu().numpy().tobytes(), tc.cpu().numpy().tobytes(), ts.cpu().numpy().tobytes()) == \
            (host.xyz.tobytes(), host.cov.tobytes(), host.score.tobytes())
        say("device form and host form agree to the bit", value=bool(same))
        b.covariance_joint(rot0, tran0)
        _, t = timed(lambda: b.covariance_joint(rot0, tran0), a.repeat)
        say(f"Batch.covariance_joint {B} x {n} with its depth rows (the host-copy route)", **t)
        full_score = host.score
        del host

    times, kept = [], 0
    for _ in range(max(1, a.repeat // 2)):
        with api.Batch(0) as b:
            b.upload(c.x1, c.x2, off, c.d12)
            t0 = time.perf_counter()
            idx, noff, thr, st = b.structure_keep_below(rot0, tran0, 0.5, 4.0)
            times.append(time.perf_counter() - t0)
            kept = len(idx)
    say(f"Batch.structure_keep_below(0.5, 4.0) {B} x {n}", ms_median=statistics.median(times) * 1e3, ms_all=[t * 1e3 for t in times],
        kept=kept, of=B * n)

    times, worst = [], 0.0
    px = torch.empty((n, 3), dtype=torch.float64, device=dev)
    pc = torch.empty((n, 6), dtype=torch.float64, device=dev)
    ps = torch.empty((n,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for _ in range(max(1, a.repeat // 2)):
        t0 = time.perf_counter()
        with api.Problem(0) as p:
            for g in range(B):
                lo, hi = g * n, (g + 1) * n
                p.upload(c.x1[lo:hi], c.x2[lo:hi], c.d12[lo:hi])
                p.structure_joint_into(px.data_ptr(), pc.data_ptr(), ps.data_ptr(), c.rot_init, c.tran_init)
                if g % 64 == 0:
                    one = ps.cpu().numpy()
                    worst = max(worst, float((np.abs(one - full_score[lo:hi]) / one).max()))
        times.append(time.perf_counter() - t0)
    say(f"{B} x (Problem.upload + Problem.structure_joint_into) at {n} matches", ms_median=statistics.median(times) * 1e3,
        ms_all=[t * 1e3 for t in times], max_rel_score_difference_to_batch=worst)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Workload for tools/profile_landmark_edit.sh: the landmark map's edits at 10^7 landmarks with half of them kept, next to the d-only
stage's pass as the yardstick of the same run, and the prune against the only route there was before it.

    python tools/landmark_edit_workload.py [n] [calls]

In ONE process (one box: boxes differ by ~6 %), on the scene of tools/landmark_fusion_workload.py:
  * 10 iterations of the d-only stage                                  -> depth_step_kernel: the YARDSTICK of the run
  * one set and one dense fuse (counts of 0 and 1)
  * `calls` scores                                                     -> landmarks_scores_kernel
  * `calls` dry prunes by a random half mask, no `kept` asked for      -> landmarks_keep_kernel alone
  * `calls` times: gather the half the mask drops (sorted indices)     -> landmarks_gather_kernel
                   prune by the mask                                   -> landmarks_keep_kernel, compact_count_kernel,
                                                                          compact_scan_kernel, landmarks_compact_scatter_kernel
                   append the gathered rows again (n is 10^7 again)    -> landmarks_append_kernel
  * `calls` times the route without these entry points: get + counts -> numpy indexing -> set (which loses the counts)
A prune uploads its n mask bytes, a gather its 8 m index bytes and downloads 76 m bytes of rows, an append uploads 72 n_add bytes: the
host-side wall times hold those copies, the kernel trace does not.  Prints one JSON line with host-side wall times; the kernel times
come from the rocprofv3 kernel trace."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from spherical_bundle_adjuster_amd import api, synthetic  # noqa: E402
from landmark_fusion_workload import covariances, timed  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out = {"n": n, "calls": calls}
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 5)
    rot, tran = c.rot_true, c.tran_true
    X = c.x1 * c.d12[:, :1]
    cov, draw = covariances(X, synthetic.BASE_SEED + 6)
    X = X + draw
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, np.full((n, 2), 5.0))
        _, sd = p.solve_depths(rot, tran, options=api.default_lm_options(max_num_iterations=10))
        out["depth_stage_us_per_pass"] = sd.seconds_total / max(sd.num_evaluations, 1) * 1e6
    rng = np.random.default_rng(synthetic.BASE_SEED + 7)
    with api.Landmarks(0) as L:
        L.set(X, cov)
        f = L.fuse(c.x2, rot, tran, 1e-3, 9.21, want_chi2=False)
        out["n_fused"] = f.n_fused
        del c, X, cov, draw
        L.scores()                                                       # first calls: occupancy queries, scratch
        out["scores_host_ms"], s = timed(calls, L.scores)
        mask = rng.random(n) < 0.5
        L.prune(mask=mask, apply=False, want_kept=False)
        out["dry_prune_host_ms"], d = timed(calls, lambda: L.prune(mask=mask, apply=False, want_kept=False))
        out["dry"] = {"n_kept": d.n_kept, "n_masked": d.n_masked, "n_invalid": d.n_invalid}
        gather_ms, prune_ms, append_ms, kept = [], [], [], []
        for _ in range(calls + 1):                                       # the first turn grows the second allocation: not timed
            mask = rng.random(n) < 0.5
            drop = np.flatnonzero(~mask).astype(np.int64)
            t, (gx, gc, gk) = timed(1, lambda: L.gather(drop))
            gather_ms.append(t)
            t, p = timed(1, lambda: L.prune(mask=mask, want_kept=False))
            prune_ms.append(t)
            kept.append(p.n_kept)
            t, _ = timed(1, lambda: L.append(gx, gc, 1.0))
            append_ms.append(t)
            assert L.size == n
        out["gather_host_ms"], out["prune_host_ms"], out["append_host_ms"] = (float(np.mean(v[1:])) for v in (gather_ms, prune_ms, append_ms))
        out["first_turn_ms"] = {"gather": gather_ms[0], "prune": prune_ms[0], "append": append_ms[0]}
        out["n_kept"] = [int(k) for k in kept[1:]]
        out["n_gathered"] = int(len(drop))

        parts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            Xh, Ch = L.get()
            kh = L.counts()
            t1 = time.perf_counter()
            Xk, Ck = Xh[mask], Ch[mask]
            t2 = time.perf_counter()
            L.set(Xk, Ck)
            t3 = time.perf_counter()
            parts.append((t1 - t0, t2 - t1, t3 - t2, t3 - t0))
            L.append(Xh[~mask], Ch[~mask], 1.0)                           # back to n for the next turn: not part of the route's time
        parts = 1e3 * np.mean(np.array(parts), axis=0)
        out["old_route_ms"] = {"get_counts": float(parts[0]), "numpy": float(parts[1]), "set": float(parts[2]), "total": float(parts[3])}
        out["result"] = {"size": L.size, "finite_scores": int(np.isfinite(s).sum()), "max_count": int(kh.max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

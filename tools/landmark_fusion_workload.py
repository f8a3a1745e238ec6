#!/usr/bin/env python3
"""Workload for tools/profile_landmark_fusion.sh: the landmark map's fusion pass at 10^7 landmarks, dense, next to the d-only
stage's pass as the yardstick of the same run.

    python tools/landmark_fusion_workload.py [n] [calls]

In ONE process (one box: boxes differ by ~6 %), on a full_rt scene (landmarks d1 * x1 drawn from a seeded covariance per landmark,
sigma_t = 0.002 |X| U(0.5, 2) across the viewing ray, sigma_r / sigma_t log-uniform in [3, 100]; bearings x2):
  * 10 iterations of the d-only stage                               -> depth_step_kernel: the YARDSTICK of the run
  * one set                                                         -> landmarks_pack_kernel
  * `calls` dry runs (apply = False) with the pose covariance       -> landmarks_fuse_kernel<false, false>
  * `calls` dry runs without it
  * `calls` fusions (apply = True; after the first, most landmarks take a second, third ... look at the same bearing)
                                                                    -> landmarks_fuse_kernel<false, true>
  * 3 indexed dry runs over every second landmark                   -> landmarks_fuse_kernel<true, false>
  * one get                                                         -> landmarks_unpack_kernel
Every fuse call uploads its 24 n bytes of bearings from the host first: the host-side wall time holds that copy, the kernel trace
does not.  Prints one JSON line with host-side wall times; the kernel times come from the rocprofv3 kernel trace."""
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
    return 1e3 * (time.perf_counter() - t0) / calls, r


def covariances(X, seed):
    """(n, 6) rows (xx, yy, zz, xy, xz, yz) and the per-landmark sigmas, built column by column to keep the peak memory low."""
    rng = np.random.default_rng(seed)
    n = len(X)
    norm = np.linalg.norm(X, axis=1)
    st = 0.002 * norm * rng.uniform(0.5, 2.0, size=n)
    sr = st * np.exp(rng.uniform(np.log(3.0), np.log(100.0), size=n))
    u = X / norm[:, None]
    rows = np.empty((n, 6))
    for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        rows[:, k] = (sr ** 2 - st ** 2) * u[:, a] * u[:, b] + (st ** 2 if a == b else 0.0)
    noise = rng.standard_normal((n, 3))
    along = np.sum(noise * u, axis=1, keepdims=True) * u
    return rows, sr[:, None] * along + st[:, None] * (noise - along)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    out = {"n": n, "calls": calls}
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 5)
    rot, tran = c.rot_true, c.tran_true
    X = c.x1 * c.d12[:, :1]
    cov, draw = covariances(X, synthetic.BASE_SEED + 6)
    X = X + draw
    pose_cov = np.diag(np.array([2e-4, 2e-4, 2e-4, 1e-3, 1e-3, 1e-3]) ** 2)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, np.full((n, 2), 5.0))
        _, sd = p.solve_depths(rot, tran, options=api.default_lm_options(max_num_iterations=10))
        out["depth_stage_us_per_pass"] = sd.seconds_total / max(sd.num_evaluations, 1) * 1e6
    with api.Landmarks(0) as L:
        out["set_ms"], _ = timed(1, lambda: L.set(X, cov))
        L.fuse(c.x2, rot, tran, 1e-3, 9.21, pose_cov, apply=False, want_chi2=False)          # first call: occupancy query, scratch
        out["dry_pose_cov_host_ms"], f = timed(calls, lambda: L.fuse(c.x2, rot, tran, 1e-3, 9.21, pose_cov, apply=False, want_chi2=False))
        out["dry_plain_host_ms"], _ = timed(calls, lambda: L.fuse(c.x2, rot, tran, 1e-3, 9.21, apply=False, want_chi2=False))
        out["first_look"] = {"n_fused": f.n_fused, "n_gated": f.n_gated, "n_behind": f.n_behind, "n_skipped": f.n_skipped}
        out["fuse_host_ms"], g = timed(calls, lambda: L.fuse(c.x2, rot, tran, 1e-3, 9.21, pose_cov, want_chi2=False))
        out["last_look"] = {"n_fused": g.n_fused, "n_gated": g.n_gated}
        idx = np.arange(0, n, 2, dtype=np.int64)
        y2 = np.ascontiguousarray(c.x2[idx])
        out["indexed_dry_host_ms"], h = timed(3, lambda: L.fuse(y2, rot, tran, 1e-3, 9.21, pose_cov, idx=idx, apply=False, want_chi2=False))
        out["indexed"] = {"m": int(len(idx)), "n_fused": h.n_fused}
        out["get_ms"], (Xg, Cg) = timed(1, L.get)
        cnt = L.counts()
        out["result"] = {"finite": bool(np.isfinite(Xg).all() and np.isfinite(Cg).all()), "max_count": int(cnt.max()),
                         "rms_before": float(np.sqrt(np.mean(np.sum(draw ** 2, axis=1)))),
                         "rms_after": float(np.sqrt(np.mean(np.sum((Xg - c.x1 * c.d12[:, :1]) ** 2, axis=1))))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

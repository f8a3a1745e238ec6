#!/usr/bin/env python3
"""Workload for tools/profile_landmark_register.sh: the joint registration of a frame against the landmark map at 10^7 landmarks,
dense, next to the d-only stage's pass and the fusion's dry run as the yardsticks of the same run.

    python tools/landmark_register_workload.py [n] [calls] [--robust] [--device-bearings] [--hampel]

In ONE process (one box: boxes differ by ~6 %), on the scene of tools/landmark_fusion_workload.py without its wrong matches (landmarks
d1 * x1 drawn from a seeded covariance per landmark; bearings x2), the start 2e-3 rad and 1e-2 units off the true pose:
  * 10 iterations of the d-only stage                               -> depth_step_kernel: the YARDSTICK of the run
  * one set, `calls` fusion dry runs without a pose covariance      -> landmarks_fuse_kernel<false, false>: the second yardstick
  * `calls` registrations as dry runs (apply = False)               -> landmarks_register_freeze_kernel<false> once per call,
                                                                       landmarks_register_reduce_kernel<false> once per evaluation,
                                                                       landmarks_register_apply_kernel<false, false> once per call
  * 3 indexed dry-run registrations over every second landmark      -> the <true> instances
  * `calls` times the SEQUENTIAL CHAIN the registration replaces, through a Problem, as a dry run as well: get_device (the dense
    frame's gather_device) -> upload_device -> set_landmark_covariances_device -> solve_resection_weighted -> resection_covariance
    -> fuse.  Its wall time against the registration's is the comparison of the speed table: against the existing route.
  * one registration with apply = True                              -> landmarks_register_apply_kernel<false, true>
Every registration and every fusion uploads its 24 n bytes of bearings from the host first, and so does the chain (once, for the
Problem): the host-side wall times hold those copies, the kernel trace does not.  Prints one JSON line with host-side wall times;
the kernel times come from the rocprofv3 kernel trace.

--robust (tools/profile_landmark_register_robust.sh): the scene WITH its wrong matches (full_rt's 5 % of bearings drawn anew), on
which the same process runs the d-only stage, one non-robust evaluation (landmarks_register_reduce_kernel<false>: the yardsticks),
then `calls` register_robust dry runs with host bearings, 3 indexed ones and one with apply = True
(landmarks_register_robust_reduce_kernel<false> / <true>), Huber delta 3, gate delta^2.  --device-bearings adds the same dry runs
with the bearings in device memory (bearings_device): the wall time without the 24 n byte upload.

--hampel (tools/profile_landmark_register_hampel.sh): see hampel_main."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from landmark_fusion_workload import covariances  # noqa: E402
from spherical_bundle_adjuster_amd import api, synthetic  # noqa: E402


def timed(calls, f):
    t0 = time.perf_counter()
    for _ in range(calls):
        r = f()
    return 1e3 * (time.perf_counter() - t0) / calls, r


def robust_main(n, calls, device_bearings):
    import torch
    delta = 3.0
    out = {"n": n, "calls": calls, "robust": True, "huber_delta": delta}
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 5)                               # with its wrong matches
    rot, tran = c.rot_true, c.tran_true
    truth = c.x1 * c.d12[:, :1]
    cov, draw = covariances(truth, synthetic.BASE_SEED + 6)
    X = truth + draw
    rng = np.random.default_rng(synthetic.BASE_SEED + 7)
    unit = lambda v: v / np.linalg.norm(v)
    rot0, tran0 = rot + 2e-3 * unit(rng.standard_normal(3)), tran + 1e-2 * unit(rng.standard_normal(3))
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, np.full((n, 2), 5.0))
        _, sd = p.solve_depths(rot, tran, options=api.default_lm_options(max_num_iterations=10))
        out["depth_stage_us_per_pass"] = sd.seconds_total / max(sd.num_evaluations, 1) * 1e6
    with api.Landmarks(0) as L:
        out["set_ms"], _ = timed(1, lambda: L.set(X, cov))
        L.eval_register(c.x2, rot0, tran0, bearing_sigma=1e-3)                           # the non-robust reduce pass: the yardstick
        out["eval_register_host_ms"], _ = timed(calls, lambda: L.eval_register(c.x2, rot0, tran0, bearing_sigma=1e-3))
        L.eval_register_robust(c.x2, rot0, tran0, delta, bearing_sigma=1e-3)
        out["eval_register_robust_host_ms"], e = timed(calls, lambda: L.eval_register_robust(c.x2, rot0, tran0, delta, bearing_sigma=1e-3))
        out["eval"] = {"n_used": e.n_used, "n_outlier": e.n_outlier}
        reg = lambda **kw: L.register_robust(c.x2, rot0, tran0, delta, 1e-3, **kw)
        reg(apply=False)                                                                 # first call: occupancy queries, scratch
        out["register_robust_dry_host_ms"], f = timed(calls, lambda: reg(apply=False))
        out["register"] = {"termination": f.summary.termination, "iterations": f.summary.num_iterations, "evaluations": f.summary.num_evaluations,
                           "seconds_eval": f.summary.seconds_eval, "n_fused": f.n_fused, "n_gated": f.n_gated, "n_used": f.n_used,
                           "n_outlier": f.n_outlier, "pose_error": [float(np.abs(f.rot - rot).max()), float(np.abs(f.tran - tran).max())]}
        idx = np.arange(0, n, 2, dtype=np.int64)
        y2 = np.ascontiguousarray(c.x2[idx])
        out["register_robust_indexed_dry_host_ms"], h = timed(3, lambda: L.register_robust(y2, rot0, tran0, delta, 1e-3, idx=idx, apply=False))
        out["indexed"] = {"m": int(len(idx)), "n_fused": h.n_fused, "evaluations": h.summary.num_evaluations}
        if device_bearings:
            ty = torch.from_numpy(np.ascontiguousarray(c.x2)).to(torch.device("cuda", 0))
            torch.cuda.synchronize()
            dreg = lambda: L.register_robust(None, rot0, tran0, delta, 1e-3, apply=False, bearings_device=ty.data_ptr(), m=n)
            g = dreg()
            out["register_robust_device_dry_host_ms"], g = timed(calls, dreg)
            out["device"] = {"evaluations": g.summary.num_evaluations, "n_fused": g.n_fused,
                             "same_pose": bool(np.array_equal(g.rot, f.rot) and np.array_equal(g.tran, f.tran))}
        out["register_robust_apply_host_ms"], a = timed(1, lambda: reg(apply=True))
        Xg, Cg = L.get()
        out["result"] = {"finite": bool(np.isfinite(Xg).all() and np.isfinite(Cg).all()), "max_count": int(L.counts().max()),
                         "n_fused": a.n_fused, "n_outlier": a.n_outlier, "rms_before": float(np.sqrt(np.mean(np.sum(draw ** 2, axis=1)))),
                         "rms_after": float(np.sqrt(np.mean(np.sum((Xg - truth) ** 2, axis=1))))}
    print(json.dumps(out))


def hampel_main(n, calls):
    """--hampel (tools/profile_landmark_register_hampel.sh): the --robust scene, bearings on the device.  ONE LOOP of `calls` rounds
    holds, interleaved, one d-only pass (depth_step_kernel), one eval_register_robust and one eval_register_hampel (their dense
    reduce kernels), so that the three kernels' times are drawn from the same stretch of the run; a second loop interleaves one
    register_robust, one register_hampel with and one without the Huber stage, all dry runs.  a = 3, b = 6, c = 12, gate a^2."""
    import torch
    a, b, c3 = 3.0, 6.0, 12.0
    out = {"n": n, "calls": calls, "hampel": True, "a": a, "b": b, "c": c3}
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 5)                               # with its wrong matches
    rot, tran = c.rot_true, c.tran_true
    truth = c.x1 * c.d12[:, :1]
    cov, draw = covariances(truth, synthetic.BASE_SEED + 6)
    X = truth + draw
    rng = np.random.default_rng(synthetic.BASE_SEED + 7)
    unit = lambda v: v / np.linalg.norm(v)
    rot0, tran0 = rot + 2e-3 * unit(rng.standard_normal(3)), tran + 1e-2 * unit(rng.standard_normal(3))
    one_pass = api.default_lm_options(max_num_iterations=1)
    with api.Problem(0) as p, api.Landmarks(0) as L:
        p.upload(c.x1, c.x2, np.full((n, 2), 5.0))
        L.set(X, cov)
        ty = torch.from_numpy(np.ascontiguousarray(c.x2)).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        dev = dict(bearings_device=ty.data_ptr(), m=n)
        ev_r = lambda: L.eval_register_robust(None, rot0, tran0, a, bearing_sigma=1e-3, **dev)
        ev_h = lambda: L.eval_register_hampel(None, rot0, tran0, a, b, c3, bearing_sigma=1e-3, **dev)
        depth = lambda: p.solve_depths(rot, tran, options=one_pass)
        depth(), ev_r(), ev_h()                                                          # first calls: occupancy queries, scratch
        t = {"depth": 0.0, "robust": 0.0, "hampel": 0.0}
        for _ in range(calls):
            for name, f in (("depth", depth), ("robust", ev_r), ("hampel", ev_h)):
                t0 = time.perf_counter()
                e = f()
                t[name] += time.perf_counter() - t0
        out["eval_host_ms"] = {k: 1e3 * v / calls for k, v in t.items()}
        out["eval"] = {"n_used": e.n_used, "n_outlier": e.n_outlier, "n_rejected": e.n_rejected}
        reg_r = lambda: L.register_robust(None, rot0, tran0, a, 1e-3, apply=False, **dev)
        reg_h = lambda: L.register_hampel(None, rot0, tran0, a, b, c3, bearing_sigma=1e-3, apply=False, **dev)
        reg_d = lambda: L.register_hampel(None, rot0, tran0, a, b, c3, huber_first=False, bearing_sigma=1e-3, apply=False, **dev)
        reg_r(), reg_h(), reg_d()
        t, last = {"robust": 0.0, "hampel_staged": 0.0, "hampel_direct": 0.0}, {}
        for _ in range(calls):
            for name, f in (("robust", reg_r), ("hampel_staged", reg_h), ("hampel_direct", reg_d)):
                t0 = time.perf_counter()
                last[name] = f()
                t[name] += time.perf_counter() - t0
        out["register_dry_host_ms"] = {k: 1e3 * v / calls for k, v in t.items()}
        err = lambda f: [float(np.abs(f.rot - rot).max()), float(np.abs(f.tran - tran).max())]
        out["register"] = {k: {"evaluations": f.summary.num_evaluations, "iterations": f.summary.num_iterations, "n_fused": f.n_fused, "n_gated": f.n_gated,
                               "n_outlier": f.n_outlier, "pose_error": err(f)} for k, f in last.items()}
        h = last["hampel_staged"]
        out["register"]["hampel_staged"].update(huber_iterations=h.huber_iterations, n_rejected=h.n_rejected)
        out["register"]["hampel_direct"].update(n_rejected=last["hampel_direct"].n_rejected)
        out["apply_host_ms"], w = timed(1, lambda: L.register_hampel(None, rot0, tran0, a, b, c3, bearing_sigma=1e-3, **dev))
        Xg, Cg = L.get()
        out["result"] = {"finite": bool(np.isfinite(Xg).all() and np.isfinite(Cg).all()), "max_count": int(L.counts().max()), "n_fused": w.n_fused,
                         "n_rejected": w.n_rejected, "rms_before": float(np.sqrt(np.mean(np.sum(draw ** 2, axis=1)))),
                         "rms_after": float(np.sqrt(np.mean(np.sum((Xg - truth) ** 2, axis=1))))}
    print(json.dumps(out))


def main():
    import torch
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    sys.argv = sys.argv[:1] + [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if set(flags) - {"--robust", "--device-bearings", "--hampel"}:
        raise SystemExit(__doc__)
    if "--hampel" in flags:
        return hampel_main(n, calls)
    if "--robust" in flags or "--device-bearings" in flags:
        return robust_main(n, calls, "--device-bearings" in flags)
    out = {"n": n, "calls": calls}
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 5, outlier_fraction=0.0)     # no wrong matches: the joint solve has no robust loss
    rot, tran = c.rot_true, c.tran_true
    truth = c.x1 * c.d12[:, :1]
    cov, draw = covariances(truth, synthetic.BASE_SEED + 6)
    X = truth + draw
    rng = np.random.default_rng(synthetic.BASE_SEED + 7)
    unit = lambda v: v / np.linalg.norm(v)
    rot0, tran0 = rot + 2e-3 * unit(rng.standard_normal(3)), tran + 1e-2 * unit(rng.standard_normal(3))
    opt = api.default_lm_options(huber_delta=0.0)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, np.full((n, 2), 5.0))
        _, sd = p.solve_depths(rot, tran, options=api.default_lm_options(max_num_iterations=10))
        out["depth_stage_us_per_pass"] = sd.seconds_total / max(sd.num_evaluations, 1) * 1e6
    dev = torch.device("cuda", 0)
    with api.Landmarks(0) as L, api.Problem(0) as q:
        out["set_ms"], _ = timed(1, lambda: L.set(X, cov))
        L.fuse(c.x2, rot, tran, 1e-3, 9.21, apply=False, want_chi2=False)                    # first call: occupancy query, scratch
        out["fuse_dry_host_ms"], _ = timed(calls, lambda: L.fuse(c.x2, rot, tran, 1e-3, 9.21, apply=False, want_chi2=False))
        reg = lambda **kw: L.register(c.x2, rot0, tran0, 1e-3, 9.21, options=opt, **kw)
        reg(apply=False)                                                                     # first call: occupancy queries, scratch
        out["register_dry_host_ms"], f = timed(calls, lambda: reg(apply=False))
        out["register"] = {"termination": f.summary.termination, "iterations": f.summary.num_iterations, "evaluations": f.summary.num_evaluations,
                           "seconds_eval": f.summary.seconds_eval, "n_fused": f.n_fused, "n_gated": f.n_gated, "n_used": f.n_used,
                           "pose_error": [float(np.abs(f.rot - rot).max()), float(np.abs(f.tran - tran).max())]}
        idx = np.arange(0, n, 2, dtype=np.int64)
        y2 = np.ascontiguousarray(c.x2[idx])
        out["register_indexed_dry_host_ms"], h = timed(3, lambda: L.register(y2, rot0, tran0, 1e-3, 9.21, idx=idx, apply=False, options=opt))
        out["indexed"] = {"m": int(len(idx)), "n_fused": h.n_fused, "evaluations": h.summary.num_evaluations}
        # the sequential chain through a Problem, on the device
        tx = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        tc = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        ones = torch.ones((n, 2), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def chain():
            L.get_device(tx.data_ptr(), tc.data_ptr())
            ty = torch.from_numpy(c.x2).to(dev)
            torch.cuda.synchronize()
            q.upload_device(tx.data_ptr(), ty.data_ptr(), ones.data_ptr(), n)
            q.set_landmark_covariances_device(tc.data_ptr(), 1.0)
            r, t, sm, _ = q.solve_resection_weighted(rot0, tran0, options=opt, bearing_sigma=1e-3, reweight_rounds=1, store_depths=False)
            cv = q.resection_covariance(r, t, opt)
            return sm, L.fuse(c.x2, r, t, 1e-3, 9.21, cv.cov, apply=False, want_chi2=False)
        chain()
        out["chain_dry_host_ms"], (sm, g) = timed(calls, chain)
        out["chain"] = {"iterations": sm.num_iterations, "evaluations": sm.num_evaluations, "n_fused": g.n_fused, "n_gated": g.n_gated}
        out["register_apply_host_ms"], a = timed(1, lambda: reg(apply=True))
        Xg, Cg = L.get()
        out["result"] = {"finite": bool(np.isfinite(Xg).all() and np.isfinite(Cg).all()), "max_count": int(L.counts().max()),
                         "n_fused": a.n_fused, "rms_before": float(np.sqrt(np.mean(np.sum(draw ** 2, axis=1)))),
                         "rms_after": float(np.sqrt(np.mean(np.sum((Xg - truth) ** 2, axis=1))))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Workload for tools/profile_resection.sh: the spherical resection's passes next to the explicit SBA_MODE_RT per-match sweep, at
10^7 per-match-depth f64 matches.

    python tools/resection_workload.py [n] [calls]

In ONE process (one box: boxes differ by ~6 %), on one handle holding a full_rt scene (landmarks d1 * x1, bearings x2):
  * `calls` eval_resection calls with the loss                     -> resect_reduce_kernel<double, true>
  * `calls` eval_resection calls without                           -> resect_reduce_kernel<double, false>
  * 3 resection_guess calls                                        -> resect_moments_kernel (+ one reduce pass without the loss)
  * 3 resection_depths calls, nothing copied to the host           -> resect_depths_kernel
  * `calls` explicit MODE_RT per-match sweeps over the folded planes (48 B / match) and `calls` over the raw planes (64 B): the
    yardsticks of the same run
  * one solve_resection from the perturbed start
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


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out = {"n": n, "calls": calls}
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 3)
    rot, tran = c.rot_init, c.tran_init
    kw = dict(depth_mode=api.DEPTH_PER_MATCH)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        loss, plain = api.default_lm_options(huber_delta=1.0), api.default_lm_options(huber_delta=0.0)
        p.eval_resection(rot, tran, loss)                                          # first call: occupancy query
        out["eval_resection_loss_host_us"], eq = timed(calls, lambda: p.eval_resection(rot, tran, loss))
        out["eval_resection_plain_host_us"], _ = timed(calls, lambda: p.eval_resection(rot, tran, plain))
        out["resection_guess_host_us"], g = timed(3, lambda: p.resection_guess())
        out["resection_depths_host_us"], _ = timed(3, lambda: p.resection_depths(rot, tran, return_depths=False))
        p.set_depths(c.d12)
        p.set_kernel(api.KERNEL_EXPLICIT)
        p.eval(api.MODE_RT, rot, tran, **kw)
        out["explicit_rt_folded_host_us"], ne = timed(calls, lambda: p.eval(api.MODE_RT, rot, tran, **kw))
        p.set_folding(False)
        p.eval(api.MODE_RT, rot, tran, **kw)
        out["explicit_rt_raw_host_us"], _ = timed(calls, lambda: p.eval(api.MODE_RT, rot, tran, **kw))
        t0 = time.perf_counter()
        r, t, sm, nb = p.solve_resection(rot, tran, loss, store_depths=False)
        out["solve_resection"] = {"ms": 1e3 * (time.perf_counter() - t0), "termination": sm.termination, "evaluations": sm.num_evaluations,
                                  "rot_err": float(np.abs(r - c.rot_true).max()), "tran_err": float(np.abs(t - c.tran_true).max()),
                                  "n_behind": nb}
        out["result"] = {"cost": eq.cost, "n_outlier": eq.n_outlier, "n_behind": eq.n_behind, "sweep_cost": ne.cost,
                         "guess_rot_err": float(np.abs(g.rot - c.rot_true).max()), "lambda2_over_lambda12": g.lambda2 / g.lambda12}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

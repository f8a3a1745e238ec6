#!/usr/bin/env python3
"""Workload for tools/profile_quantile.sh: a data-derived inlier cut at 10^7 per-match-depth f64 matches and at 256 pairs of
50 000, by the host route and by the device route.

    python tools/quantile_workload.py [n] [reps] [pairs] [pair_n]

Per rep, single problem: the host route -- residuals(fields=("sq_norm",)) (8 B per match to the host), np.partition at the
median, a byte mask sq_norm <= scale * median, compact(mask) (1 B per match back) -- then, on a fresh upload, the device
route keep_below(0.5, scale); both must keep the same matches.  Then one residual_quantiles call with 5 probabilities.  The
same for the batch.  Prints one JSON line with host-side wall times (medians, ms); kernel times come from the kernel trace."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from spherical_bundle_adjuster_amd import api, synthetic  # noqa: E402

SCALE = 4.0
PROBS = [0.0, 0.25, 0.5, 0.9, 1.0]


def single(n, reps):
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 2, outlier_fraction=0.1)
    kw = dict(depth_mode=api.DEPTH_PER_MATCH)
    t = {"host_route": [], "device_route": [], "quantiles_5": []}
    kept = 0
    with api.Problem(0) as p:
        for _ in range(reps):
            p.upload(c.x1, c.x2, c.d12)
            t0 = time.perf_counter()
            s = p.residuals(c.rot_init, c.tran_init, fields=("sq_norm",), **kw).sq_norm
            k = (n - 1) // 2
            thr_h = SCALE * np.partition(s, k)[k]
            idx_h = p.compact(s <= thr_h)
            t1 = time.perf_counter()
            p.upload(c.x1, c.x2, c.d12)
            t2 = time.perf_counter()
            idx_d, thr_d = p.keep_below(c.rot_init, c.tran_init, 0.5, SCALE, **kw)
            t3 = time.perf_counter()
            assert thr_d == thr_h and np.array_equal(idx_d, idx_h)
            p.upload(c.x1, c.x2, c.d12)
            t4 = time.perf_counter()
            p.residual_quantiles(c.rot_init, c.tran_init, PROBS, **kw)
            t5 = time.perf_counter()
            kept = int(idx_d.shape[0])
            t["host_route"].append(t1 - t0)
            t["device_route"].append(t3 - t2)
            t["quantiles_5"].append(t5 - t4)
    return {"n": n, "kept": kept, "host_ms_median": {k: 1e3 * float(np.median(v)) for k, v in t.items()}}


def batch(B, n, reps):
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 3, outlier_fraction=0.1)
    rng = np.random.default_rng(2)
    perm = np.concatenate([rng.permutation(n) for _ in range(B)])
    x1, x2, d12 = c.x1[perm], c.x2[perm], c.d12[perm]
    off = (np.arange(B + 1) * n).astype(np.uint64)
    rot, tran = np.tile(c.rot_init, (B, 1)), np.tile(c.tran_init, (B, 1))
    kw = dict(depth_mode=api.DEPTH_PER_MATCH)
    t = {"host_route": [], "device_route": [], "quantiles_5": []}
    kept = 0
    with api.Batch(0) as b:
        for _ in range(reps):
            b.upload(x1, x2, off, d12)
            t0 = time.perf_counter()
            s = b.residuals(rot, tran, fields=("sq_norm",), **kw).sq_norm.reshape(B, n)
            k = (n - 1) // 2
            thr_h = SCALE * np.partition(s, k, axis=1)[:, k]
            idx_h, _ = b.compact((s <= thr_h[:, None]).reshape(-1))
            t1 = time.perf_counter()
            b.upload(x1, x2, off, d12)
            t2 = time.perf_counter()
            idx_d, _, thr_d = b.keep_below(rot, tran, 0.5, SCALE, **kw)
            t3 = time.perf_counter()
            assert np.array_equal(thr_d, thr_h) and np.array_equal(idx_d, idx_h)
            b.upload(x1, x2, off, d12)
            t4 = time.perf_counter()
            b.residual_quantiles(rot, tran, PROBS, **kw)
            t5 = time.perf_counter()
            kept = int(idx_d.shape[0])
            t["host_route"].append(t1 - t0)
            t["device_route"].append(t3 - t2)
            t["quantiles_5"].append(t5 - t4)
    return {"pairs": B, "pair_n": n, "kept": kept, "host_ms_median": {k: 1e3 * float(np.median(v)) for k, v in t.items()}}


def main():
    a = [int(v) for v in sys.argv[1:]]
    n, reps, B, pn = (a + [10_000_000, 5, 256, 50_000][len(a):])[:4]
    print(json.dumps({"reps": reps, "scale": SCALE, "single": single(n, reps), "batch": batch(B, pn, reps)}))


if __name__ == "__main__":
    main()

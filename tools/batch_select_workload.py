#!/usr/bin/env python3
"""Workload for tools/profile_batch_select.sh: a batch's per-match residuals and compaction at config C5 (256 pairs x 50 k
per-match-depth f64 matches).

    python tools/batch_select_workload.py [pairs] [matches_per_pair] [reps]

Per rep: one count-only residual call (the kernel reads the 64 B/match planes, coordinates and depths, and writes the
per-pair counts), one call that returns e, sq_norm and inlier (+33 B/match written), a compaction keeping a random 50 %
(1 B keep + 64 B of planes read per match, 64 B written per kept match), then keep_inliers against
residuals(fields=("inlier",)) + compact on fresh uploads of the full batch; one batched step (sba_batch_eval) per rep reads
the same planes for comparison.  Prints one JSON line with host-side wall times
(the uploads in between are not timed); the kernel times come from the rocprofv3 kernel trace."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from spherical_bundle_adjuster_amd import api, synthetic  # noqa: E402


def main():
    pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    m = int(sys.argv[2]) if len(sys.argv) > 2 else 50_000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    c = synthetic.full_rt(pairs * m, seed=synthetic.BASE_SEED + 2)
    off = (np.arange(pairs + 1) * m).astype(np.uint64)
    rot = np.tile(c.rot_init, (pairs, 1))
    tran = np.tile(c.tran_init, (pairs, 1))
    keep = np.random.default_rng(1).random(pairs * m) < 0.5
    dm = api.DEPTH_PER_MATCH
    t = {"count_only": [], "all_outputs": [], "compact": [], "keep_inliers": [], "residuals_inlier_then_compact": []}
    with api.Batch(0) as b:
        b.upload(c.x1, c.x2, off, c.d12)
        bpp = b.blocks_per_pair
        for _ in range(reps):
            b.upload(c.x1, c.x2, off, c.d12)
            b.eval(api.MODE_RT, rot, tran, huber_delta=1.0, depth_mode=dm)     # the batched step over the same planes
            t0 = time.perf_counter()
            r0 = b.residuals(rot, tran, huber_delta=1.0, depth_mode=dm, fields=())
            t1 = time.perf_counter()
            r1 = b.residuals(rot, tran, huber_delta=1.0, depth_mode=dm)
            t2 = time.perf_counter()
            idx, _ = b.compact(keep)
            t3 = time.perf_counter()
            assert np.array_equal(r0.n_inlier, r1.n_inlier) and idx.size == int(keep.sum())
            b.upload(c.x1, c.x2, off, c.d12)
            t4 = time.perf_counter()
            ki, _ = b.keep_inliers(rot, tran, huber_delta=1.0, depth_mode=dm)
            t5 = time.perf_counter()
            b.upload(c.x1, c.x2, off, c.d12)
            t6 = time.perf_counter()
            r = b.residuals(rot, tran, huber_delta=1.0, depth_mode=dm, fields=("inlier",))
            ci, _ = b.compact(r.inlier)
            t7 = time.perf_counter()
            assert np.array_equal(ki, ci)
            t["count_only"].append(t1 - t0)
            t["all_outputs"].append(t2 - t1)
            t["compact"].append(t3 - t2)
            t["keep_inliers"].append(t5 - t4)
            t["residuals_inlier_then_compact"].append(t7 - t6)
    print(json.dumps({"pairs": pairs, "matches_per_pair": m, "reps": reps, "kept": int(keep.sum()),
                      "n_inlier": int(r1.n_inlier.sum()), "blocks_per_pair": bpp,
                      "host_ms_median": {k: 1e3 * float(np.median(v)) for k, v in t.items()}}))


if __name__ == "__main__":
    main()

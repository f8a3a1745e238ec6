#!/usr/bin/env python3
"""Workload for tools/profile_select.sh: per-match residuals and compaction at 10^7 per-match-depth f64 matches.

    python tools/select_workload.py [n] [reps]

Per rep: one count-only residual call (the kernel reads the 48 B/match folded planes and writes nothing else), one call
that returns e, sq_norm and inlier (+33 B/match written), then a compaction keeping a random 50 % (1 B keep + 64 B of planes
read per match, 64 B written per kept match), after which the full problem is uploaded again.  Prints one JSON line with
host-side wall times; the kernel times come from the rocprofv3 kernel trace."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from spherical_bundle_adjuster_amd import api, synthetic  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 2)
    keep = np.random.default_rng(1).random(n) < 0.5
    t = {"count_only": [], "all_outputs": [], "compact": []}
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        for _ in range(reps):
            t0 = time.perf_counter()
            r0 = p.residuals(c.rot_init, c.tran_init, huber_delta=1.0, depth_mode=api.DEPTH_PER_MATCH, fields=())
            t1 = time.perf_counter()
            r1 = p.residuals(c.rot_init, c.tran_init, huber_delta=1.0, depth_mode=api.DEPTH_PER_MATCH)
            t2 = time.perf_counter()
            idx = p.compact(keep)
            t3 = time.perf_counter()
            assert r0.n_inlier == r1.n_inlier and idx.size == int(keep.sum())
            t["count_only"].append(t1 - t0)
            t["all_outputs"].append(t2 - t1)
            t["compact"].append(t3 - t2)
            p.upload(c.x1, c.x2, c.d12)
    print(json.dumps({"n": n, "reps": reps, "kept": int(keep.sum()), "n_inlier": r1.n_inlier,
                      "host_ms_median": {k: 1e3 * float(np.median(v)) for k, v in t.items()}}))


if __name__ == "__main__":
    main()

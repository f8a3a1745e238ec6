#!/bin/bash
# Run on a machine with an MI355X: kernel trace of tools/batch_covariance_workload.py (config C5: 256 pairs x 50 000 per-match
# f64 matches through Batch.covariance_joint, and in the SAME run the route it replaces: 256 x Problem.upload +
# Problem.covariance_joint), then batch_cov_kernel's per-launch time with and without the depth phase and its rate on the
# algorithmic bytes, counted from the code (f64 planes, per match):
#   reduce + finish           6 coordinate + 2 depth planes read = 64 B
#   reduce + finish + depth   the same 64 B read twice + 3 doubles written = 152 B
# The launches are told apart by their order in the workload: per driver one warm-up call, then `repeat` calls with the depth
# phase, then `repeat` without; the lock-step driver's launches (two per call with the depth phase) are listed separately.
set -o pipefail
# usage: tools/profile_batch_covariance.sh OUT_DIR   (trace and summary go there)
OUT=${1:?usage: tools/profile_batch_covariance.sh OUT_DIR}
PAIRS=${PAIRS:-256}
MATCHES=${MATCHES:-50000}
REPEAT=${REPEAT:-5}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- python3 tools/batch_covariance_workload.py \
  --pairs $PAIRS --matches $MATCHES --repeat $REPEAT > $OUT/workload.jsonl 2> $OUT/workload.err &&
timeout -k 10 120 python3 - "$OUT" "$PAIRS" "$MATCHES" "$REPEAT" <<'PY'
import csv, glob, json, statistics, sys
out, B, n, rep = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
for line in open(f"{out}/workload.jsonl"):
    print(line.rstrip())
rows = []
for f in glob.glob(f"{out}/trace/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
def durs(name):
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
d = durs("batch_cov_kernel")
# device driver: 1 warm-up + rep with depths + rep without; lock-step: 2 warm-up + 2 rep (reduce, depth alternating) + rep (reduce)
want = (1 + 2 * rep) + (2 + 3 * rep)
groups = []
if len(d) == want:
    groups = [("one launch: reduce+finish+depth", d[1:1 + rep], 152), ("one launch: reduce+finish", d[1 + rep:1 + 2 * rep], 64)]
    ls = d[1 + 2 * rep:]
    groups += [("lock-step: reduce launch", ls[2:2 + 2 * rep:2] + ls[2 + 2 * rep:], 64), ("lock-step: depth launch", ls[3:2 + 2 * rep:2], 88)]
else:
    print(f"batch_cov_kernel: {len(d)} launches traced, {want} expected: not split by phase")
    groups = [("batch_cov_kernel (all launches)", d, 0)]
print(f"{'launch':34s} {'calls':>5s} {'mean us':>9s} {'min us':>9s} {'max us':>9s} {'B/match':>8s} {'GB/s mean':>10s} {'(at min)':>9s}")
for name, g, b in groups:
    if not g:
        print(f"{name:34s} none traced"); continue
    m = statistics.mean(g)
    print(f"{name:34s} {len(g):5d} {m:9.1f} {min(g):9.1f} {max(g):9.1f} {b:8d} {b * B * n / (m * 1e3):10.1f} {b * B * n / (min(g) * 1e3):9.1f}")
for name in ("cov_reduce_kernel", "cov_depth_kernel", "cov_finalize_kernel"):
    g = durs(name)
    if g:
        print(f"{name:34s} {len(g):5d} {statistics.mean(g):9.1f} {min(g):9.1f} {max(g):9.1f}   (the single-problem route, {n} matches per launch)")
PY
rc=$?
if [ $rc -ne 0 ]; then echo "trace failed ($rc)" >&2; tail -5 $OUT/workload.err >&2; fi
exit $rc

#!/bin/bash
# Run on a machine with an MI355X: kernel trace of tools/batch_select_workload.py (a batch's per-match residuals and
# compaction at config C5: 256 pairs x 50 k per-match f64 matches), then each kernel's mean time and its rate on the
# algorithmic bytes:
#   batch_residual_kernel, count only   64 B read per match (coordinate and depth planes)
#   batch_residual_kernel, all outputs  64 B read + 33 B written per match (e 24, sq_norm 8, inlier 1)
#   batch_residual_kernel, inlier only  64 B read + 1 B written per match (keep_inliers and residuals(fields=("inlier",)))
#   compaction (count + scan + pair count + scatter)   1 B + 64 B read per match, 64 B written per kept match
set -o pipefail
# usage: tools/profile_batch_select.sh OUT_DIR   (trace and summary go there)
OUT=${1:?usage: tools/profile_batch_select.sh OUT_DIR}
PAIRS=${PAIRS:-256}
M=${M:-50000}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- \
  python3 tools/batch_select_workload.py $PAIRS $M 5 > $OUT/workload.json 2> $OUT/workload.err || { echo "trace failed" >&2; exit 1; }
python3 - "$OUT" "$PAIRS" "$M" <<'PY'
import csv, glob, json, statistics, sys
out, pairs, m = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
n = pairs * m
w = json.load(open(f"{out}/workload.json"))
rows = []
for f in glob.glob(f"{out}/trace/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
def durs(pred):
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if pred(r["Kernel_Name"])]
def res(flag):
    return lambda k: "batch_residual_kernel<" in k and k.split("batch_residual_kernel<")[1].split(">")[0].endswith(", " + flag)
groups = {
    "batch_residual_kernel count only": (durs(res("0")), 64 * n),
    "batch_residual_kernel all outputs": (durs(res("7")), 97 * n),
    "batch_residual_kernel inlier only": (durs(res("4")), 65 * n),
    "compact_count_kernel": (durs(lambda k: "compact_count_kernel" in k and "batch" not in k), 1 * n),
    "compact_scan_kernel": (durs(lambda k: "compact_scan_kernel" in k), 0),
    "batch_pair_kept_kernel": (durs(lambda k: "batch_pair_kept_kernel" in k), 0),
    "batch_compact_scatter_kernel": (durs(lambda k: "batch_compact_scatter_kernel" in k), None),
    "batch_step_kernel (the uploads' reference)": (durs(lambda k: "batch_step_kernel" in k), 64 * n),
}
print(f"pairs = {pairs} x {m} = {n} per-match f64 matches, workload: {json.dumps(w)}")
print(f"{'kernel':44s} {'calls':>5s} {'mean us':>9s} {'min us':>9s} {'max us':>9s} {'GB/s (mean)':>12s}")
for name, (d, b) in groups.items():
    if not d:
        print(f"{name:44s} none traced"); continue
    mean = statistics.mean(d)
    rate = "" if not b else f"{b / (mean * 1e3):12.1f}"
    print(f"{name:44s} {len(d):5d} {mean:9.1f} {min(d):9.1f} {max(d):9.1f} {rate:>12s}")
# every compaction scatters the kept rows: 50 % (compact) or the inliers (keep_inliers, residuals + compact)
sc = groups["batch_compact_scatter_kernel"][0]
if sc:
    print("scatter calls in workload order (us):", " ".join(f"{x:.1f}" for x in sc))
PY

#!/bin/bash
# Run on a machine with an MI355X: kernel trace of tools/select_workload.py (per-match residuals and compaction at 10^7 per-match f64
# matches), then each kernel's mean time and its rate on the algorithmic bytes:
#   residual_kernel, count only   48 B read per match (the folded planes)
#   residual_kernel, all outputs  48 B read + 33 B written per match (e 24, sq_norm 8, inlier 1)
#   compaction (count + scan + scatter)   1 B + 64 B read per match, 64 B written per kept match
set -o pipefail
# usage: tools/profile_select.sh OUT_DIR   (trace and summary go there)
OUT=${1:?usage: tools/profile_select.sh OUT_DIR}
N=${N:-10000000}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- python3 tools/select_workload.py $N 5 \
  > $OUT/workload.json 2> $OUT/workload.err || { echo "trace failed" >&2; exit 1; }
python3 - "$OUT" "$N" <<'PY'
import csv, glob, json, statistics, sys
out, n = sys.argv[1], int(sys.argv[2])
w = json.load(open(f"{out}/workload.json"))
kept = w["kept"]
rows = []
for f in glob.glob(f"{out}/trace/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
def durs(pred):
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if pred(r["Kernel_Name"])]
groups = {
    "residual_kernel count only": (durs(lambda k: "residual_kernel<" in k and k.split("residual_kernel<")[1].split(">")[0].endswith(", 0")), 48 * n),
    "residual_kernel all outputs": (durs(lambda k: "residual_kernel<" in k and k.split("residual_kernel<")[1].split(">")[0].endswith(", 7")), 81 * n),
    "compact_count_kernel": (durs(lambda k: "compact_count_kernel" in k), 1 * n),
    "compact_scan_kernel": (durs(lambda k: "compact_scan_kernel" in k), 0),
    "compact_scatter_kernel": (durs(lambda k: "compact_scatter_kernel" in k), 65 * n + 64 * kept),
}
print(f"n = {n}, kept = {kept} (compaction), workload: {json.dumps(w)}")
print(f"{'kernel':32s} {'calls':>5s} {'mean us':>9s} {'min us':>9s} {'max us':>9s} {'GB/s (mean)':>12s}")
for name, (d, b) in groups.items():
    if not d:
        print(f"{name:32s} none traced"); continue
    m = statistics.mean(d)
    print(f"{name:32s} {len(d):5d} {m:9.1f} {min(d):9.1f} {max(d):9.1f} {(b / (m * 1e3) if b else 0):12.1f}")
c = groups["compact_count_kernel"][0]; s = groups["compact_scan_kernel"][0]; sc = groups["compact_scatter_kernel"][0]
if c and s and sc:
    tot = statistics.mean(c) + statistics.mean(s) + statistics.mean(sc)
    print(f"{'compaction (3 kernels)':32s} {'':5s} {tot:9.1f} {'':9s} {'':9s} {(65 * n + 64 * kept) / (tot * 1e3):12.1f}")
PY

#!/bin/bash
# Run on a machine with an MI355X: kernel trace of tools/batch_structure_workload.py (config C5: 256 pairs x 50 000 per-match
# f64 matches through Batch.structure_joint_into / structure_joint / structure_keep_below, and in the SAME run the routes they
# replace: 256 x Problem.upload + Problem.structure_joint_into, and Batch.covariance_joint with its depth rows), then
# batch_structure_kernel's per-launch time for all outputs and for the score alone, batch_cov_kernel's in the same run, and
# their rates on the algorithmic bytes, counted from the code (f64 planes, per match):
#   batch_structure_kernel, all outputs   6 coordinate + 2 depth planes read = 64 B, 3 + 6 + 1 doubles written = 80 B: 144 B
#   batch_structure_kernel, score only    64 B read, 8 B written: 72 B
#   batch_cov_kernel, reduce + finish     64 B read
# The instantiations are told apart by their template arguments in the traced kernel name.
set -o pipefail
# usage: tools/profile_batch_structure.sh OUT_DIR   (trace and summary go there)
OUT=${1:?usage: tools/profile_batch_structure.sh OUT_DIR}
PAIRS=${PAIRS:-256}
MATCHES=${MATCHES:-50000}
REPEAT=${REPEAT:-5}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- python3 tools/batch_structure_workload.py \
  --pairs $PAIRS --matches $MATCHES --repeat $REPEAT > $OUT/workload.jsonl 2> $OUT/workload.err &&
timeout -k 10 120 python3 - "$OUT" "$PAIRS" "$MATCHES" <<'PY'
import csv, glob, statistics, sys
out, B, n = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
for line in open(f"{out}/workload.jsonl"):
    print(line.rstrip())
rows = []
for f in glob.glob(f"{out}/trace/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
def durs(name, *either):
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows
            if name in r["Kernel_Name"] and (not either or any(e in r["Kernel_Name"].replace(" ", "") for e in either))]
groups = [("batch_structure_kernel<all outputs>", durs("batch_structure_kernel", "true,true,true>", "Lb1ELb1ELb1E"), 144),
          ("batch_structure_kernel<score only>", durs("batch_structure_kernel", "false,false,true>", "Lb0ELb0ELb1E"), 72),
          ("batch_cov_kernel (every launch)", durs("batch_cov_kernel"), 0)]
print(f"{'launch':38s} {'calls':>5s} {'mean us':>9s} {'median':>9s} {'min us':>9s} {'max us':>9s} {'B/match':>8s} {'GB/s mean':>10s} {'(at min)':>9s}")
for name, g, b in groups:
    if not g:
        print(f"{name:38s} none traced"); continue
    m = statistics.mean(g)
    rate = f"{b * B * n / (m * 1e3):10.1f} {b * B * n / (min(g) * 1e3):9.1f}" if b else ""
    print(f"{name:38s} {len(g):5d} {m:9.1f} {statistics.median(g):9.1f} {min(g):9.1f} {max(g):9.1f} {b:8d} {rate}")
for name in ("structure_kernel", "cov_reduce_kernel", "select_hist", "keep_below", "order_stats"):
    g = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows
         if name in r["Kernel_Name"] and "batch_structure_kernel" not in r["Kernel_Name"]]
    if g:
        print(f"{name:38s} {len(g):5d} {statistics.mean(g):9.1f} {statistics.median(g):9.1f} {min(g):9.1f} {max(g):9.1f}")
PY
rc=$?
if [ $rc -ne 0 ]; then echo "trace failed ($rc)" >&2; tail -5 $OUT/workload.err >&2; fi
exit $rc

#!/bin/bash
# Run on a machine with an MI355X: kernel trace of tools/resection_weighted_workload.py (the covariance-weighted resection at 10^7
# per-match f64 matches, with the unweighted resect_reduce_kernel in the SAME run as the baseline), then each kernel's per-launch
# mean / minimum and its rate on the algorithmic bytes, counted from the code (f64 planes, per match):
#   resect_reduce_kernel        6 coordinate planes + d1 read = 56 B                          (the baseline)
#   resect_wreduce_kernel       56 B + the three weight planes = 80 B read; the covariance rows are never read
#   resect_weights_kernel       56 B + the covariance row 48 B read, 24 B written = 128 B
#   resect_weight_rows_kernel   the three bearing planes 24 B + 24 B read, 48 B written = 96 B
# A kernel trace of its own: no counters in the same run.
set -o pipefail
# usage: tools/profile_resection_weighted.sh OUT_DIR   (trace and summary go there)
OUT=${1:?usage: tools/profile_resection_weighted.sh OUT_DIR}
N=${N:-10000000}
CALLS=${CALLS:-20}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- python3 tools/resection_weighted_workload.py $N $CALLS \
  > $OUT/workload.json 2> $OUT/workload.err &&
timeout -k 10 120 python3 - "$OUT" "$N" <<'PY'
import csv, glob, json, statistics, sys
out, n = sys.argv[1], int(sys.argv[2])
w = json.load(open(f"{out}/workload.json"))
rows = []
for f in glob.glob(f"{out}/trace/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
def durs(names):
    d = [((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0))
         for r in rows if any(s in r["Kernel_Name"] for s in names)]
    if d:      # the launches over the whole problem
        g = max(x[1] for x in d)
        d = [x for x in d if x[1] == g]
    return [x[0] for x in d]
PEAK = 8000.0   # GB/s
# a kernel's name as the trace spells it: demangled, or mangled
groups = [("resect_reduce_kernel loss", ("resect_reduce_kernel<double, true>", "resect_reduce_kernelIdLb1E"), 56),
          ("resect_reduce_kernel plain", ("resect_reduce_kernel<double, false>", "resect_reduce_kernelIdLb0E"), 56),
          ("resect_wreduce_kernel loss", ("resect_wreduce_kernel<double, true>", "resect_wreduce_kernelIdLb1E"), 80),
          ("resect_wreduce_kernel plain", ("resect_wreduce_kernel<double, false>", "resect_wreduce_kernelIdLb0E"), 80),
          ("resect_weights_kernel", ("resect_weights_kernel",), 128), ("resect_weight_rows_kernel", ("resect_weight_rows_kernel",), 96),
          ("joint_finalize_kernel", ("joint_finalize_kernel",), 0)]
print(f"n = {n}; workload: {json.dumps(w)}")
print(f"{'kernel':28s} {'calls':>5s} {'mean us':>9s} {'min us':>9s} {'max us':>9s} {'B/match':>8s} {'GB/s mean':>10s} {'of 8 TB/s':>9s} {'(at min)':>9s}")
for label, names, b in groups:
    d = durs(names)
    if not d:
        print(f"{label:28s} none traced"); continue
    m = statistics.mean(d)
    bw = b * n / (m * 1e3) if b else 0.0
    bwmin = b * n / (min(d) * 1e3) if b else 0.0
    print(f"{label:28s} {len(d):5d} {m:9.1f} {min(d):9.1f} {max(d):9.1f} {b:8d} {bw:10.1f} {bw / PEAK:9.2f} {bwmin / PEAK:9.2f}")
PY
rc=$?
if [ $rc -ne 0 ]; then echo "trace failed ($rc)" >&2; tail -5 $OUT/workload.err >&2; fi
exit $rc

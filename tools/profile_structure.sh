#!/bin/bash
# Run on a machine with an MI355X: kernel trace of tools/structure_workload.py (the triangulated structure at 10^7 per-match f64
# matches, with the covariance's depth pass and the d-only stage in the SAME run as yardsticks), then each kernel's per-launch
# mean / minimum and its rate on the algorithmic bytes, counted from the code (f64 planes, per match):
#   structure_kernel, all outputs   6 coordinate + 2 depth planes read = 64 B, xyz 24 B + cov 48 B + score 8 B written = 144 B
#   structure_kernel, score only    64 B read + 8 B written = 72 B
#   cov_reduce_kernel               64 B read
#   cov_depth_kernel                64 B read + 3 doubles written = 88 B
#   depth_step_kernel               8 planes + 2 scaling planes read, 2 candidate planes written = 96 B (first pass: + 16 B written)
set -o pipefail
# usage: tools/profile_structure.sh OUT_DIR   (trace and summary go there)
OUT=${1:?usage: tools/profile_structure.sh OUT_DIR}
N=${N:-10000000}
CALLS=${CALLS:-20}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- python3 tools/structure_workload.py $N $CALLS \
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
# a kernel's name as the trace spells it: demangled, or mangled (template arguments <double, xyz, cov, score>)
groups = [("structure_kernel all", ("structure_kernel<double, true, true, true>", "structure_kernelIdLb1ELb1ELb1E"), 144),
          ("structure_kernel score", ("structure_kernel<double, false, false, true>", "structure_kernelIdLb0ELb0ELb1E"), 72),
          ("cov_reduce_kernel", ("cov_reduce_kernel",), 64), ("cov_depth_kernel", ("cov_depth_kernel",), 88),
          ("cov_finalize_kernel", ("cov_finalize_kernel",), 0), ("depth_step_kernel", ("depth_step_kernel",), 96)]
print(f"n = {n}; workload: {json.dumps(w)}")
print(f"{'kernel':26s} {'calls':>5s} {'mean us':>9s} {'min us':>9s} {'max us':>9s} {'B/match':>8s} {'GB/s mean':>10s} {'of 8 TB/s':>9s} {'(at min)':>9s}")
for label, names, b in groups:
    d = durs(names)
    if not d:
        print(f"{label:26s} none traced"); continue
    m = statistics.mean(d)
    bw = b * n / (m * 1e3) if b else 0.0
    bwmin = b * n / (min(d) * 1e3) if b else 0.0
    print(f"{label:26s} {len(d):5d} {m:9.1f} {min(d):9.1f} {max(d):9.1f} {b:8d} {bw:10.1f} {bw / PEAK:9.2f} {bwmin / PEAK:9.2f}")
PY
rc=$?
if [ $rc -ne 0 ]; then echo "trace failed ($rc)" >&2; tail -5 $OUT/workload.err >&2; fi
exit $rc

#!/bin/bash
# Run on a machine with an MI355X: kernel trace of tools/landmark_register_workload.py --hampel (the joint registration under
# Hampel's loss at 10^7 landmarks on the scene with its wrong matches, bearings on the device).  The workload holds
# depth_step_kernel, landmarks_register_robust_reduce_kernel and landmarks_register_hampel_reduce_kernel INTERLEAVED IN ONE LOOP, so
# the three are compared over the same stretch of one run.  Per kernel: per-launch mean / minimum / maximum and the rate on the
# algorithmic bytes, counted from the code (per landmark):
#   depth_step_kernel                                 8 planes + 2 scaling planes read, 2 candidate planes written = 96 B   (the yardstick)
#   landmarks_register_robust_reduce_kernel dense     72 + 24 + 8 B read = 104 B                                             (the yardstick)
#   landmarks_register_hampel_reduce_kernel dense     72 + 24 + 8 B read = 104 B
# and the wall time of one register_hampel dry run with and without its Huber stage against one register_robust dry run.  A
# kernel trace of its own: no counters in the same run.  The summary goes to OUT_DIR/landmark_register_hampel_kernels.log (the copy
# kept in the repository: profiles/landmark_register_hampel_kernels.log).
set -o pipefail
# usage: tools/profile_landmark_register_hampel.sh OUT_DIR   (trace and summary go there)
OUT=${1:?usage: tools/profile_landmark_register_hampel.sh OUT_DIR}
N=${N:-10000000}
CALLS=${CALLS:-5}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- python3 tools/landmark_register_workload.py $N $CALLS \
  --hampel > $OUT/workload.json 2> $OUT/workload.err &&
timeout -k 10 120 python3 - "$OUT" "$N" <<'PY' | tee $OUT/landmark_register_hampel_kernels.log
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
groups = [("depth_step_kernel", ("depth_step_kernel",), 96, n),
          ("robust_reduce dense", ("landmarks_register_robust_reduce_kernel<false>", "landmarks_register_robust_reduce_kernelILb0EE"), 104, n),
          ("hampel_reduce dense", ("landmarks_register_hampel_reduce_kernel<false>", "landmarks_register_hampel_reduce_kernelILb0EE"), 104, n)]
print(f"n = {n}; workload: {json.dumps(w)}")
print(f"{'kernel':28s} {'calls':>5s} {'mean us':>9s} {'median':>9s} {'min us':>9s} {'max us':>9s} {'B/item':>8s} {'GB/s mean':>10s} {'of 8 TB/s':>9s} {'(at min)':>9s}")
means = {}
for label, names, b, items in groups:
    d = durs(names)
    if not d:
        print(f"{label:28s} none traced"); continue
    m = statistics.mean(d)
    means[label] = (m, statistics.median(d), min(d))
    bw = b * items / (m * 1e3)
    bwmin = b * items / (min(d) * 1e3)
    print(f"{label:28s} {len(d):5d} {m:9.1f} {statistics.median(d):9.1f} {min(d):9.1f} {max(d):9.1f} {b:8d} {bw:10.1f} {bw / PEAK:9.2f} {bwmin / PEAK:9.2f}")
if "robust_reduce dense" in means and "hampel_reduce dense" in means:
    r, h = means["robust_reduce dense"], means["hampel_reduce dense"]
    print(f"hampel_reduce / robust_reduce: mean {h[0] / r[0]:.3f}, median {h[1] / r[1]:.3f}, minimum {h[2] / r[2]:.3f}")
t, g = w["register_dry_host_ms"], w["register"]
print(f"wall time, dry runs with device bearings: register_robust {t['robust']:.2f} ms ({g['robust']['evaluations']} evaluations), register_hampel "
      f"with its Huber stage {t['hampel_staged']:.2f} ms ({g['hampel_staged']['huber_iterations']} Huber iterations, then "
      f"{g['hampel_staged']['evaluations']} evaluations), without {t['hampel_direct']:.2f} ms ({g['hampel_direct']['evaluations']} evaluations)")
PY
rc=$?
if [ $rc -ne 0 ]; then echo "trace failed ($rc)" >&2; tail -5 $OUT/workload.err >&2; fi
exit $rc

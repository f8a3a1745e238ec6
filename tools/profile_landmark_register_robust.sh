#!/bin/bash
# Run on a machine with an MI355X: kernel trace of tools/landmark_register_workload.py --robust --device-bearings (the robust joint
# registration at 10^7 landmarks on the scene with its wrong matches, with depth_step_kernel and the non-robust reduce pass in the
# SAME run as the yardsticks), then each kernel's per-launch mean / minimum and its rate on the algorithmic bytes, counted from
# the code (per landmark):
#   depth_step_kernel                                 8 planes + 2 scaling planes read, 2 candidate planes written = 96 B   (the yardstick)
#   landmarks_register_reduce_kernel dense            72 + 24 + 8 B read = 104 B                                             (the yardstick)
#   landmarks_register_robust_reduce_kernel dense     72 + 24 + 8 B read = 104 B
#   landmarks_register_robust_reduce_kernel indexed   per OBSERVATION: 72 B gathered + 8 B index + 24 B bearing + 8 B noise = 112 B
# and the wall time of one register_robust dry run with host bearings against one with device bearings.  A kernel trace of its
# own: no counters in the same run.  The summary goes to OUT_DIR/landmark_register_robust_kernels.log (the copy kept in the
# repository: profiles/landmark_register_robust_kernels.log).
set -o pipefail
# usage: tools/profile_landmark_register_robust.sh OUT_DIR   (trace and summary go there)
OUT=${1:?usage: tools/profile_landmark_register_robust.sh OUT_DIR}
N=${N:-10000000}
CALLS=${CALLS:-5}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- python3 tools/landmark_register_workload.py $N $CALLS \
  --robust --device-bearings > $OUT/workload.json 2> $OUT/workload.err &&
timeout -k 10 120 python3 - "$OUT" "$N" <<'PY' | tee $OUT/landmark_register_robust_kernels.log
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
m_idx = w.get("indexed", {}).get("m", n // 2)
# a kernel's name as the trace spells it: demangled, or mangled
groups = [("depth_step_kernel", ("depth_step_kernel",), 96, n),
          ("register_reduce dense", ("landmarks_register_reduce_kernel<false>", "landmarks_register_reduce_kernelILb0EE"), 104, n),
          ("robust_reduce dense", ("landmarks_register_robust_reduce_kernel<false>", "landmarks_register_robust_reduce_kernelILb0EE"), 104, n),
          ("robust_reduce indexed", ("landmarks_register_robust_reduce_kernel<true>", "landmarks_register_robust_reduce_kernelILb1EE"), 112, m_idx),
          ("register_freeze dense", ("landmarks_register_freeze_kernel<false>", "landmarks_register_freeze_kernelILb0EE"), 104, n),
          ("register_apply dense dry", ("landmarks_register_apply_kernel<false, false>", "landmarks_register_apply_kernelILb0ELb0E"), 104, n)]
print(f"n = {n}; workload: {json.dumps(w)}")
print(f"{'kernel':28s} {'calls':>5s} {'mean us':>9s} {'min us':>9s} {'max us':>9s} {'B/item':>8s} {'GB/s mean':>10s} {'of 8 TB/s':>9s} {'(at min)':>9s}")
for label, names, b, items in groups:
    d = durs(names)
    if not d:
        print(f"{label:28s} none traced"); continue
    m = statistics.mean(d)
    bw = b * items / (m * 1e3)
    bwmin = b * items / (min(d) * 1e3)
    print(f"{label:28s} {len(d):5d} {m:9.1f} {min(d):9.1f} {max(d):9.1f} {b:8d} {bw:10.1f} {bw / PEAK:9.2f} {bwmin / PEAK:9.2f}")
dev = w.get("register_robust_device_dry_host_ms")
print(f"wall time, dry runs: one register_robust with host bearings {w['register_robust_dry_host_ms']:.2f} ms ({w['register']['evaluations']} "
      f"evaluations), with device bearings " + (f"{dev:.2f} ms ({w['device']['evaluations']} evaluations)" if dev is not None else "not run"))
PY
rc=$?
if [ $rc -ne 0 ]; then echo "trace failed ($rc)" >&2; tail -5 $OUT/workload.err >&2; fi
exit $rc

#!/bin/bash
# Run on a machine with an MI355X: kernel trace of tools/landmark_fusion_workload.py (the landmark map's fusion pass at 10^7
# landmarks, dense, with depth_step_kernel in the SAME run as the yardstick), then each kernel's per-launch mean / minimum and its
# rate on the algorithmic bytes, counted from the code (per landmark):
#   depth_step_kernel                8 planes + 2 scaling planes read, 2 candidate planes written = 96 B     (the yardstick)
#   landmarks_fuse_kernel dense dry  9 planes 72 B + the bearing row 24 B read = 96 B
#   landmarks_fuse_kernel dense      72 + 4 (count) + 24 B read, up to 72 + 4 B written = 176 B when every landmark is fused
#   landmarks_fuse_kernel indexed dry   per OBSERVATION: 72 B gathered + 8 B index + 24 B bearing = 104 B
#   landmarks_pack_kernel            72 B of rows read, 76 B of planes written = 148 B
#   landmarks_unpack_kernel          72 B of planes read, 72 B of rows written = 144 B
# (no chi2 is asked for in the workload: 8 B per landmark more when it is).  A kernel trace of its own: no counters in the same run.
set -o pipefail
# usage: tools/profile_landmark_fusion.sh OUT_DIR   (trace and summary go there)
OUT=${1:?usage: tools/profile_landmark_fusion.sh OUT_DIR}
N=${N:-10000000}
CALLS=${CALLS:-10}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- python3 tools/landmark_fusion_workload.py $N $CALLS \
  > $OUT/workload.json 2> $OUT/workload.err &&
timeout -k 10 120 python3 - "$OUT" "$N" <<'PY'
import csv, glob, json, statistics, sys
out, n = sys.argv[1], int(sys.argv[2])
w = json.load(open(f"{out}/workload.json"))
rows = []
for f in glob.glob(f"{out}/trace/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
def durs(names, part=None):
    d = [((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0), int(r["Start_Timestamp"]))
         for r in rows if any(s in r["Kernel_Name"] for s in names)]
    if d:      # the launches over the whole problem, in the order they ran
        g = max(x[1] for x in d)
        d = sorted((x for x in d if x[1] == g), key=lambda x: x[2])
    if part is not None:      # the workload's dry runs: 1 + calls with the pose covariance, then calls without it
        d = d[:w["calls"] + 1] if part == 0 else d[w["calls"] + 1:]
    return [x[0] for x in d]
PEAK = 8000.0   # GB/s
m_idx = w.get("indexed", {}).get("m", n // 2)
DRY = ("landmarks_fuse_kernel<false, false>", "landmarks_fuse_kernelILb0ELb0E")
# a kernel's name as the trace spells it: demangled, or mangled
groups = [("depth_step_kernel", ("depth_step_kernel",), 96, n),
          ("landmarks_fuse dense dry", DRY, 96, n),
          ("landmarks_fuse dense apply", ("landmarks_fuse_kernel<false, true>", "landmarks_fuse_kernelILb0ELb1E"), 176, n),
          ("landmarks_fuse indexed dry", ("landmarks_fuse_kernel<true, false>", "landmarks_fuse_kernelILb1ELb0E"), 104, m_idx),
          ("landmarks_pack_kernel", ("landmarks_pack_kernel",), 148, n), ("landmarks_unpack_kernel", ("landmarks_unpack_kernel",), 144, n)]
print(f"n = {n}; workload: {json.dumps(w)}")
print(f"{'kernel':28s} {'calls':>5s} {'mean us':>9s} {'min us':>9s} {'max us':>9s} {'B/item':>8s} {'GB/s mean':>10s} {'of 8 TB/s':>9s} {'(at min)':>9s}")
groups[2:2] = [("  ... with Sigma_pose", DRY, 96, n, 0), ("  ... without it", DRY, 96, n, 1)]
for label, names, b, items, *part in groups:
    d = durs(names, *part)
    if not d:
        print(f"{label:28s} none traced"); continue
    m = statistics.mean(d)
    bw = b * items / (m * 1e3)
    bwmin = b * items / (min(d) * 1e3)
    print(f"{label:28s} {len(d):5d} {m:9.1f} {min(d):9.1f} {max(d):9.1f} {b:8d} {bw:10.1f} {bw / PEAK:9.2f} {bwmin / PEAK:9.2f}")
PY
rc=$?
if [ $rc -ne 0 ]; then echo "trace failed ($rc)" >&2; tail -5 $OUT/workload.err >&2; fi
exit $rc

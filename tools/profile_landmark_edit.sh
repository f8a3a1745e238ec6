#!/bin/bash
# Run on a machine with an MI355X: kernel trace of tools/landmark_edit_workload.py (the landmark map's edits at 10^7 landmarks with
# half of them kept, with depth_step_kernel in the SAME run as the yardstick), then each kernel's per-launch mean / minimum and its
# rate on the algorithmic bytes, counted from the code (per landmark of the map unless said otherwise):
#   depth_step_kernel                 8 planes + 2 scaling planes read, 2 candidate planes written = 96 B     (the yardstick)
#   landmarks_scores_kernel           9 planes 72 B read, 8 B written = 80 B
#   landmarks_keep_kernel             72 + 4 (count) + 1 (mask) B read, 1 keep byte written = 78 B
#   compact_count_kernel              1 keep byte read
#   compact_scan_kernel               12 B per tile of 2048 landmarks: one block, a latency
#   landmarks_compact_scatter_kernel  1 keep byte + the lines of all ten planes 76 B read, 76 B written per KEPT landmark
#                                     = 77 + 76 * (kept fraction) B
#   landmarks_append_kernel           per landmark of the NEW layout 76 B written; read 76 B per old landmark, 72 B per new row
#   landmarks_gather_kernel           per ROW: 8 B index + 76 B gathered + 76 B written = 160 B
# A kernel trace of its own: no counters in the same run.  The wall times of the workload (its JSON line) hold the host copies.
set -o pipefail
# usage: tools/profile_landmark_edit.sh OUT_DIR   (trace and summary go there)
OUT=${1:?usage: tools/profile_landmark_edit.sh OUT_DIR}
N=${N:-10000000}
CALLS=${CALLS:-5}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- python3 tools/landmark_edit_workload.py $N $CALLS \
  > $OUT/workload.json 2> $OUT/workload.err &&
timeout -k 10 120 python3 - "$OUT" "$N" <<'PY'
import csv, glob, json, statistics, sys
out, n = sys.argv[1], int(sys.argv[2])
w = json.load(open(f"{out}/workload.json"))
rows = []
for f in glob.glob(f"{out}/trace/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
def durs(name, skip_first):
    d = [((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0), int(r["Start_Timestamp"]))
         for r in rows if name in r["Kernel_Name"]]
    if d:      # the launches over the whole map, in the order they ran
        g = max(x[1] for x in d)
        d = sorted((x for x in d if x[1] == g), key=lambda x: x[2])
    return [x[0] for x in d][skip_first:]
PEAK = 8000.0   # GB/s
kept = statistics.mean(w["n_kept"]) / n
m = w["n_gathered"]
# bytes per item, items; the first launch of a kernel that also pays for a growing allocation's first touch is left out where noted
groups = [("depth_step_kernel", "depth_step_kernel", 96, n, 0),
          ("landmarks_scores_kernel", "landmarks_scores_kernel", 80, n, 1),
          ("landmarks_keep_kernel", "landmarks_keep_kernel", 78, n, 1),
          ("compact_count_kernel", "compact_count_kernel", 1, n, 1),
          ("compact_scan_kernel", "compact_scan_kernel", 12 / 2048, n, 1),
          ("landmarks_compact_scatter", "landmarks_compact_scatter_kernel", 77 + 76 * kept, n, 1),
          ("landmarks_append_kernel", "landmarks_append_kernel", 76 + 76 * kept + 72 * (1 - kept), n, 1),
          ("landmarks_gather_kernel", "landmarks_gather_kernel", 160, m, 1)]
print(f"n = {n}, kept fraction {kept:.4f}, gathered rows {m}; workload: {json.dumps(w)}")
print(f"{'kernel':28s} {'calls':>5s} {'mean us':>9s} {'min us':>9s} {'max us':>9s} {'B/item':>8s} {'GB/s mean':>10s} {'of 8 TB/s':>9s} {'(at min)':>9s}")
for label, name, b, items, skip in groups:
    d = durs(name, skip)
    if not d:
        print(f"{label:28s} none traced"); continue
    mean = statistics.mean(d)
    bw = b * items / (mean * 1e3)
    bwmin = b * items / (min(d) * 1e3)
    print(f"{label:28s} {len(d):5d} {mean:9.1f} {min(d):9.1f} {max(d):9.1f} {b:8.1f} {bw:10.1f} {bw / PEAK:9.2f} {bwmin / PEAK:9.2f}")
r = w["old_route_ms"]
print(f"prune, wall: {w['prune_host_ms']:.1f} ms (mask upload, keep, count, scan, scatter, two waits); the route without it, wall: "
      f"{r['total']:.1f} ms = get + counts {r['get_counts']:.1f} + numpy {r['numpy']:.1f} + set {r['set']:.1f} (and the counts are lost)")
print(f"gather of {m} rows, wall: {w['gather_host_ms']:.1f} ms; append of as many, wall: {w['append_host_ms']:.1f} ms; scores, wall: "
      f"{w['scores_host_ms']:.1f} ms; dry prune, wall: {w['dry_prune_host_ms']:.1f} ms")
PY
rc=$?
if [ $rc -ne 0 ]; then echo "trace failed ($rc)" >&2; tail -5 $OUT/workload.err >&2; fi
exit $rc

#!/bin/bash
# Run on a machine with an MI355X: tools/quantile_workload.py (an inlier cut from the data at 10^7 per-match f64 matches and at
# 256 x 50 000, host route against device route) once for the wall times, then once more under a kernel trace of its own for
# each kernel's mean time and its rate on the algorithmic bytes per match:
#   residual_kernel, sq_norm only     48 B read (the folded planes) + 8 B written: HBM-bound, the in-run yardstick
#   select_hist_kernel                8 B read; from the second pass on the 80 MB plane sits in the Infinity Cache
#   keep_below_kernel                 8 B read + 1 B written
# usage: tools/profile_quantile.sh OUT_DIR   (trace and summary go there)
set -o pipefail
OUT=${1:?usage: tools/profile_quantile.sh OUT_DIR}
N=${N:-10000000}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 420 python3 tools/quantile_workload.py $N 5 > $OUT/wall.json 2> $OUT/wall.err || { echo "workload failed" >&2; tail -5 $OUT/wall.err >&2; exit 1; }
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- python3 tools/quantile_workload.py $N 3 \
  > $OUT/workload.json 2> $OUT/workload.err || { echo "trace failed" >&2; exit 1; }
python3 - "$OUT" "$N" <<'PY'
import csv, glob, json, statistics, sys
out, n = sys.argv[1], int(sys.argv[2])
w = json.load(open(f"{out}/wall.json"))
rows = []
for f in glob.glob(f"{out}/trace/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
def durs(pred):
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if pred(r["Kernel_Name"])]
single = lambda k: "batch_" not in k
sq_only = lambda k: k.split("residual_kernel<")[1].split(">")[0].endswith(", 2")
print("wall times, not traced (ms, medians):", json.dumps(w))
for what, ratio in (("single", w["single"]["host_ms_median"]), ("batch", w["batch"]["host_ms_median"])):
    print(f"{what}: host route {ratio['host_route']:.1f} ms, device route {ratio['device_route']:.1f} ms, "
          f"x{ratio['host_route'] / ratio['device_route']:.1f}")
# the hist kernel's launches alternate single / batch per rep and the passes differ: split the single problem's by grid size
hist = [r for r in rows if "select_hist_kernel" in r["Kernel_Name"]]
groups = {
    "residual_kernel sq_norm only (single)": (durs(lambda k: "residual_kernel<" in k and single(k) and sq_only(k)), 56),
    "batch_residual_kernel sq_norm only": (durs(lambda k: "batch_residual_kernel<" in k and sq_only(k)), 72),
    "select_hist_kernel (all passes, both)": (durs(lambda k: "select_hist_kernel" in k), 8),
    "select_narrow_kernel": (durs(lambda k: "select_narrow_kernel" in k), 0),
    "keep_below_kernel": (durs(lambda k: "keep_below_kernel" in k), 9),
}
print(f"{'kernel':40s} {'calls':>5s} {'mean us':>9s} {'min us':>9s} {'max us':>9s} {'B/match':>8s} {'GB/s (mean)':>12s}")
for name, (d, b) in groups.items():
    if not d:
        print(f"{name:40s} none traced"); continue
    m = statistics.mean(d)
    rows_n = n if "batch" not in name else w["batch"]["pairs"] * w["batch"]["pair_n"]
    print(f"{name:40s} {len(d):5d} {m:9.1f} {min(d):9.1f} {max(d):9.1f} {b:8d} {(b * rows_n / (m * 1e3) if b else 0):12.1f}")
# pass by pass (launch order within one selection: 8 passes)
by_grid = {}
for r in hist:
    by_grid.setdefault(r.get("Grid_Size", r.get("Grid_Size_X", "?")), []).append(r)
for g, rs in by_grid.items():
    rs.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_pass = [[] for _ in range(8)]
    for i, r in enumerate(rs):
        per_pass[i % 8].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"select_hist_kernel grid {g}: mean us per pass " + " ".join(f"{statistics.mean(p):.1f}" for p in per_pass if p))
PY

#!/bin/bash
# Run on a machine with an MI355X: kernel trace of tools/landmark_associate_workload.py -- one associate_device call at a map-sized
# shape (10^6 landmarks x 8 192 frame rows x D = 64), sba_match_descriptors_device alone on the same arrays (what claim +
# compaction + gather add on top), the host route the association replaces (match, numpy unique, sort, upload), and a prune of
# half a described map at 10^7 x 64 next to the same prune undescribed -- then each kernel's per-launch mean / minimum.  Bytes,
# counted from the code:
#   landmarks_claim_kernel                 per accepted frame row 12 B read, one 8-byte atomic
#   landmarks_associate_keep_kernel        per landmark 8 B read, 1 keep byte written
#   landmarks_associate_scatter_kernel     per landmark 1 keep byte; per claimed landmark 8 + 24 B read, 16 + 24 B written
#   landmarks_desc_compact_scatter_kernel  per landmark 1 keep byte; per KEPT landmark 4 dim B read and written
# A kernel trace of its own: no counters in the same run.  The wall times of the workload (its JSON line) hold the host copies.
set -o pipefail
# usage: tools/profile_landmark_associate.sh OUT_DIR   (trace and summary go there; the summary also to profiles/landmark_associate_kernels.log)
OUT=${1:?usage: tools/profile_landmark_associate.sh OUT_DIR}
N=${N:-1000000}
M=${M:-8192}
DIM=${DIM:-64}
NPRUNE=${NPRUNE:-10000000}
CALLS=${CALLS:-5}
mkdir -p $OUT profiles
export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- python3 tools/landmark_associate_workload.py $N $M $DIM $NPRUNE $CALLS \
  > $OUT/workload.json 2> $OUT/workload.err &&
timeout -k 10 120 python3 - "$OUT" <<'PY' | tee profiles/landmark_associate_kernels.log
import csv, glob, json, statistics, sys
out = sys.argv[1]
w = json.load(open(f"{out}/workload.json"))
rows = []
for f in glob.glob(f"{out}/trace/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
print(f"workload: {json.dumps(w)}")
print(f"{'kernel':42s} {'calls':>5s} {'mean us':>9s} {'min us':>9s} {'max us':>9s}")
for name in ("match_pack_kernel", "match_tiles_kernel", "match_finish_kernel", "match_scatter_kernel", "landmarks_claim_kernel",
             "landmarks_associate_keep_kernel", "compact_count_kernel", "compact_scan_kernel", "landmarks_associate_scatter_kernel",
             "landmarks_keep_kernel", "landmarks_compact_scatter_kernel", "landmarks_desc_compact_scatter_kernel"):
    d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
    if not d:
        print(f"{name:42s} none traced"); continue
    print(f"{name:42s} {len(d):5d} {statistics.mean(d):9.1f} {min(d):9.1f} {max(d):9.1f}")
kept, dim = w["n_kept"], w["dim"]
d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "landmarks_desc_compact_scatter_kernel" in r["Kernel_Name"]]
if d:
    b = w["n_prune"] + 8.0 * dim * kept
    print(f"landmarks_desc_compact_scatter_kernel: {b / (statistics.mean(d) * 1e3):.1f} GB/s on {b / 1e9:.2f} GB = {b / (statistics.mean(d) * 1e3) / 8000.0:.2f} of 8 TB/s")
print(f"associate_device {w['associate_device_ms']:.3f} ms, the matcher alone {w['match_device_alone_ms']:.3f} ms, associate from host rows "
      f"{w['associate_host_ms']:.3f} ms, the host route {w['host_route_ms']:.3f} ms; prune described {w['prune_described_ms']:.3f} ms, "
      f"undescribed {w['prune_undescribed_ms']:.3f} ms")
PY

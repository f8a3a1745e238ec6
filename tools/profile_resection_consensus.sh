#!/bin/bash
# Run on a machine with an MI355X: kernel trace of tools/resection_consensus_workload.py (the robust resection guess at 10^7
# per-match f64 matches), then per kernel the per-launch mean / minimum and
#   resect_score_kernel            picoseconds per match and candidate, at 128 and at 1024 candidates, next to the expectation
#                                  written down before the first run: 23 f64 vector instructions per match and candidate in the
#                                  generated code (12 for c = Rn X + t, 4 for d*, 3 for r, 3 for |r|^2, the compare) at the
#                                  device's f64 vector rate, 78.6 TFLOP/s = 39.3 * 10^12 instruction lanes per second
#                                  (256 CUs x 4 SIMDs x 16 lanes per clock x 2.4 GHz): 0.59 ps, 6.0 ms for 10^7 x 1024;
#                                  its 56 B per match are read once for ALL candidates (0.1 ms): compute-bound from ~20 candidates
#   resect_inlier_moments_kernel   the refit pass next to resect_moments_kernel of the same run, both on 56 B per match; expected
#                                  at the moments pass's fraction of the bandwidth (0.65 of 8 TB/s, profiles/resection_kernels.log):
#                                  23 more instructions per match do not move a bandwidth-bound pass
#   the whole consensus call       its wall time, the kernels' share of it, and the rest: the host's (128 trials, copies, waits)
# The launches of the score kernel are told apart by their order in the trace: the workload's warm-up call, `calls` with 128
# candidates, `calls` with 1024, then per consensus call the trials' launch and the refit's single candidate.
# A kernel trace of its own: no counters in the same run.
set -o pipefail
# usage: tools/profile_resection_consensus.sh OUT_DIR   (trace and summary go there)
OUT=${1:?usage: tools/profile_resection_consensus.sh OUT_DIR}
N=${N:-10000000}
CALLS=${CALLS:-5}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o t -- python3 tools/resection_consensus_workload.py $N $CALLS \
  > $OUT/workload.json 2> $OUT/workload.err &&
timeout -k 10 120 python3 - "$OUT" "$N" "$CALLS" <<'PY'
import csv, glob, json, statistics, sys
out, n, calls = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
w = json.load(open(f"{out}/workload.json"))
rows = []
for f in glob.glob(f"{out}/trace/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
def durs(name):
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
PEAK, RATE = 8000.0, 39.3e12   # GB/s; f64 vector instruction lanes per second
print(f"n = {n}; workload: {json.dumps(w)}")
score = durs("resect_score_kernel")
groups = [("score, 128 candidates", score[1:1 + calls], 128), ("score, 1024 candidates", score[1 + calls:1 + 2 * calls], 1024),
          ("score, consensus trials", score[1 + 2 * calls::2], w["result"]["valid_trials"]), ("score, the refit alone", score[2 + 2 * calls::2], 1)]
print(f"{'resect_score_kernel':28s} {'calls':>5s} {'mean us':>10s} {'min us':>10s} {'ps/match/cand':>14s} {'(at min)':>9s} {'expected':>9s} {'of f64 rate':>11s}")
for label, d, k in groups:
    if not d:
        print(f"{label:28s} none traced"); continue
    m = statistics.mean(d)
    ps, psmin = m * 1e6 / (n * k), min(d) * 1e6 / (n * k)
    print(f"{label:28s} {len(d):5d} {m:10.1f} {min(d):10.1f} {ps:14.3f} {psmin:9.3f} {23e12 / RATE:9.3f} {23e12 / RATE / ps:11.2f}")
print(f"{'kernel':28s} {'calls':>5s} {'mean us':>10s} {'min us':>10s} {'B/match':>8s} {'GB/s mean':>10s} {'of 8 TB/s':>9s} {'(at min)':>9s}")
for label, name, b in (("resect_inlier_moments_kernel", "resect_inlier_moments_kernel", 56), ("resect_moments_kernel", "resect_moments_kernel", 56),
                       ("resect_reduce_kernel plain", "resect_reduce_kernel", 56), ("resect_gather_kernel", "resect_gather_kernel", 0),
                       ("joint_finalize_kernel", "joint_finalize_kernel", 0)):
    d = durs(name)
    if not d:
        print(f"{label:28s} none traced"); continue
    m = statistics.mean(d)
    print(f"{label:28s} {len(d):5d} {m:10.1f} {min(d):10.1f} {b:8d} {b * n / (m * 1e3):10.1f} {b * n / (m * 1e3) / PEAK:9.2f} {b * n / (min(d) * 1e3) / PEAK:9.2f}")
per_call = sum(statistics.mean(d) for d in (groups[2][1], groups[3][1], durs("resect_inlier_moments_kernel"), durs("resect_gather_kernel")) if d)
per_call += statistics.mean(durs("resect_reduce_kernel")[-3:] or [0.0])
wall = w["consensus_host_us"]
print(f"consensus call: wall {wall:.1f} us, its kernels {per_call:.1f} us ({per_call / wall:.2f}), the host's share {wall - per_call:.1f} us "
      f"(sampling, 128 trials, copies, launches and waits)")
PY
rc=$?
if [ $rc -ne 0 ]; then echo "trace failed ($rc)" >&2; tail -5 $OUT/workload.err >&2; fi
exit $rc

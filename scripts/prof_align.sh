# usage: bash scripts/prof_align.sh [rows] [out_dir]  -> share of the align kernels in rnamc_bpp_alignment
# One kernel-trace run (no counters) of scripts/align_time.py --skip-b: a warm-up and one repetition of
# route (a) at one size; the kernels' total durations by name, the three align kernels among them.
set -e
HERE=$(cd "$(dirname "$0")/.." && pwd)
ROWS=${1:-200}
OUT=${2:-${TMPDIR:-/tmp}/trace_align_$ROWS}
rm -rf "$OUT" && mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT" -- python3 "$HERE/scripts/align_time.py" --rows "$ROWS" --reps 1 --skip-b > "$OUT/run.log" 2>&1
cat "$OUT/run.log"
python3 - "$OUT" <<'PY'
import csv, glob, os, re, sys
out = sys.argv[1]
f = sorted(glob.glob(out + "/**/*kernel_stats.csv", recursive=True), key=os.path.getmtime)[-1]
rows = list(csv.DictReader(open(f)))
total = sum(float(r["TotalDurationNs"]) for r in rows)
mine = [r for r in rows if "k_align_" in r["Name"]]
line = open(out + "/run.log").read()
wall = [float(x) for x in re.findall(r"\(a\) rnamc_bpp_alignment\s+([0-9.]+) s", line)]
print("kernels in the trace: %d names, %.1f ms in all (two calls of route (a) and the context warm-up)" % (len(rows), total / 1e6))
for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:12]:
    print("  %-60s calls %7s total %10.3f ms" % (r["Name"][:60], r["Calls"], float(r["TotalDurationNs"]) / 1e6))
for r in mine:
    print("  %-60s calls %7s total %10.3f ms" % (r["Name"][:60], r["Calls"], float(r["TotalDurationNs"]) / 1e6))
a = sum(float(r["TotalDurationNs"]) for r in mine)
print("align kernels: %.3f ms = %.2f %% of the kernel time" % (a / 1e6, 100 * a / total))
if wall:
    print("per call (two calls traced): %.3f ms of %.3f s wall (traced) = %.2f %% of the call" % (a / 2e6, wall[0], 100 * a / 2e9 / wall[0]))
PY
find "$OUT" -name "*kernel_trace.csv" -delete

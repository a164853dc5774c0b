# usage: bash scripts/prof_duplex_pmc.sh [out_dir]  -> hardware counters of the duplex kernels
# Counter passes only (no tracing domains), each a run of its own, of scripts/duplex_time.py --trace 1:
# two scan-form calls under Turner (22-nt query x batch[:1000]); the counters summed per kernel.
HERE=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-${TMPDIR:-/tmp}/pmc_duplex}
rm -rf "$OUT" && mkdir -p "$OUT"
i=0
for SET in \
 "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU" \
 "SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VALU_TRANS SQ_THREAD_CYCLES_VALU" \
 "TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum TCC_EA0_RDREQ_sum GRBM_GUI_ACTIVE" \
; do
  i=$((i+1))
  timeout -k 10 240 rocprofv3 --pmc $SET --output-format csv -d "$OUT/p$i" -- python3 "$HERE/scripts/duplex_time.py" --trace 1 > "$OUT/run$i.log" 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then
    echo "pass $i ($SET) failed, rc=$rc"; tail -5 "$OUT/run$i.log"
    if [ $rc -ge 124 ]; then exit $rc; fi  # killed or timed out: nothing more on the device
  fi
done
grep -h "calls, wall" "$OUT/run1.log"
python3 - "$OUT" <<'PY' | tee "$OUT/summary.txt"
import collections, csv, glob, sys
out = sys.argv[1]
agg = collections.defaultdict(lambda: collections.defaultdict(float))
for f in glob.glob(out + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        kn = r["Kernel_Name"]
        if "k_duplex_" not in kn:
            continue
        agg["k_duplex_" + kn.split("k_duplex_")[1].split("(")[0]][r["Counter_Name"]] += float(r["Counter_Value"])
for k, v in sorted(agg.items()):
    print(k)
    for c, x in sorted(v.items()):
        print(f"   {c:32s} {x:.6g}")
PY
find "$OUT" -name "*counter_collection.csv" -delete

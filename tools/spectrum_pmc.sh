#!/bin/bash
# tools/spectrum_pmc.sh [OUT_DIR] -- hardware counters of the spectrum kernels on the workload of tools/spectrum_rate.py at 200
# tracks, the kernels alone: one `rocprofv3 --pmc` pass per counter group, never combined with a trace, then the mean per
# dispatch of every counter and kernel (profiles/spectrum_pmc.txt).
set -o pipefail
O=${1:-profiles/spectrum_pmc}
rm -rf "$O"; mkdir -p "$O"
i=0
for grp in "SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU" \
           "SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS" \
           "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE" "GRBM_GUI_ACTIVE" "FETCH_SIZE"; do
  i=$((i+1))
  timeout -k 10 150 rocprofv3 --pmc $grp -d "$O/g$i" --output-format csv -- python tools/spectrum_rate.py --no-torch --tracks 200 --reps 2 \
      --warm-ms 0 --host-tracks 0 --json - > "$O/g$i.log" 2>&1 || { echo "group $i failed"; tail -5 "$O/g$i.log"; exit 1; }
done
python - "$O" <<'PY' | tee "$O/summary.txt"
import collections
import csv
import glob
import sys

acc = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(sys.argv[1] + "/g*/**/*counter_collection.csv", recursive=True):
    for row in csv.DictReader(open(f)):
        k = row["Kernel_Name"]
        if "rg_spec_tiles" in k or "rg_spec_fold" in k:
            acc[k[:60]][row["Counter_Name"]].append(float(row["Counter_Value"]))
for k in sorted(acc):
    print(k)
    for n in sorted(acc[k]):
        v = acc[k][n]
        print(f"  {n:28s} {sum(v) / len(v):18.1f}  (n={len(v)})")
PY

#!/bin/bash
# L2 read requests of the CUs (TCP_TCC_READ_REQ_sum) per decode-GEMM launch of a 64-row step of the BAIR-size GPT, weights row-major
# (CCVS_DECODE_TILED_W=0) against tiled (1): profiles/gemm_tiled_operands.txt.  Eager steps (a counter pass cannot follow graph
# replays), one counter per pass, kernel trace only.  Each pass runs once under its own time limit; the first failure ends the script.
#   bash tools/gemm_tiled_pmc.sh [rows] [tokens] [output directory]
ROWS=${1:-64}; TOK=${2:-30}; OUT=${3:-/tmp/gemm_tiled_pmc}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$OUT"
export CCVS_PROBE_EAGER=1
for v in 0 1; do
  rm -rf "$OUT/pmc_$v"
  CCVS_DECODE_TILED_W=$v timeout -k 10 300 rocprofv3 --kernel-trace --pmc TCP_TCC_READ_REQ_sum -d "$OUT/pmc_$v" -o p --output-format csv -- \
      python3 "$ROOT/tools/token_step_probe.py" "$TOK" "$ROWS" > "$OUT/pmc_$v.log" 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then tail -n 20 "$OUT/pmc_$v.log"; echo "counter pass (tiled=$v) failed: $rc"; exit $rc; fi
done
python3 - "$OUT" <<'PY'
import collections, csv, glob, sys
csv.field_size_limit(1 << 30)
for v in (0, 1):
    cnt, n = collections.defaultdict(float), collections.defaultdict(int)
    for f in glob.glob(f"{sys.argv[1]}/pmc_{v}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "gemm16_kernel" not in r["Kernel_Name"] or r["Counter_Name"] != "TCP_TCC_READ_REQ_sum":
                continue
            grid = ".".join(str(r.get(k, "?")) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z")) if "Grid_Size_X" in r else r.get("Grid_Size", "?")
            key = (r["Kernel_Name"].split("(")[0].replace("void ", ""), grid)
            cnt[key] += float(r["Counter_Value"])
            n[key] += 1
    launches = max(sum(n.values()), 1)
    print(f"CCVS_DECODE_TILED_W={v}: {launches} gemm16 launches, TCP_TCC_READ_REQ_sum {sum(cnt.values()) / launches / 1e3:.1f} k per launch")
    for key in sorted(cnt, key=lambda k: -n[k]):
        print(f"   {key[0]}  grid (threads) {key[1]:>14s}  {n[key]:6d} x  {cnt[key] / n[key] / 1e3:9.1f} k")
PY

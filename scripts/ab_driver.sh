#!/bin/bash
# scripts/ab_driver.sh "<label> ENV=VAL ..." ...: the driver's own invocation (--steps 20 --warmup 5) under each environment
# (--full: the line also carries the other modes' ms / step); results in $OUT (default ab_out/)
OUT=${OUT:-ab_out}; mkdir -p "$OUT"
for spec in "$@"; do
  set -- $spec; label=$1; shift
  ( for kv in "$@"; do export "$kv"; done
    python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline > "$OUT/abd_$label.json" 2> "$OUT/abd_$label.err"
    python - <<PY
import json
try:
    d = json.loads(open("$OUT/abd_$label.json").read().strip().splitlines()[-1]); print("$label", d["ms_per_step"], d.get("modes_ms_per_step"))
except Exception as e:
    print("$label", "FAILED", e)
PY
  )
done

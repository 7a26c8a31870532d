#!/bin/bash
# The driver's own command on this lease, kept as it prints (quote what the driver will see):
#   tools/driver_style.sh <tag> [out_dir]      -> <out_dir>/driver_style.json  (one JSON line; run it on three leases, commit min / median / max)
# --full: the summary below reads the cold_call and host_api blocks, which a plain run leaves out.
TAG=${1:-driver_style}
OUT=${2:-bench_runs/$TAG}
mkdir -p "$OUT"
python bench.py --full --gpus 1 --steps 20 --warmup 5 > "$OUT/driver_style.json" 2> "$OUT/driver_style.err"
python - <<PY
import json
d = json.loads(open("$OUT/driver_style.json").read().strip().splitlines()[-1])
print({k: d[k] for k in ("value", "ms_per_step")}, d["roofline"]["frac"], d["roofline"]["kernel_ms_avg"], d.get("cold_call"), d["host_api"]["rows_per_s"], d["detail"]["csr_upload_s"])
PY

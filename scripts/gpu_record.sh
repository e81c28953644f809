#!/bin/bash
# record run: bench.py --full (with cpu_baseline), then rocprofv3 stats + PMC passes of a short bench.  Logs -> $OUT (default results/)
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT:-results}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
timeout 1200 python bench.py --full > "$OUT/bench_default.log" 2> "$OUT/bench_default.err"
echo "bench exit $?" >> "$OUT/bench_default.err"
STEPS=10 bash scripts/gpu_profile.sh > "$OUT/profile.log" 2>&1
python - "$OUT" <<'PY'
import json, os, sys
for l in open(os.path.join(sys.argv[1], 'bench_default.log')):
    if l.startswith('{'):
        d = json.loads(l); print({k: d[k] for k in ('value', 'ms_per_step', 'steps')}, d['config']['mean_accept_len'], d['roofline']['frac'], d['roofline']['verify_step']['frac'], d['cpu_baseline']['value'], d['cpu_baseline']['ms_per_step'])
PY
grep -E "^== (FETCH|WRITE)|^void k_|^k_" "$OUT/profile.log" | cut -c1-150 | head -40

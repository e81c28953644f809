#!/bin/bash
# A/B of the single-launch tree attention's forms (la_lab_set key 37, csrc/la_attn1.hip) on the headline leg, both arms in the LAB build:
#   scripts/gpu_attn1_dv_ab.sh [form ...]          (default: 20 = SL 1, DV 4, the library default; arm A is always 37=0, the SL = 2, DV = 1 form)
# Alternating visits of bench.py --steps 48 --warmup 6 (VISITS per arm, default 3), then one rocprofv3 --kernel-trace --stats run per arm.
# Every GPU step runs under its own time limit and the script stops at the first step that fails.
set -u -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-results}; mkdir -p "$OUT"
FORMS=${*:-20}
VISITS=${VISITS:-3}
TAB=$OUT/attn1_dv_ab.txt
: > "$TAB"
visit() {      # label, knob value
  LA_DEBUG="37=$2" timeout -k 10 240 python bench.py --gpus 1 --steps 48 --warmup 6 > "$OUT/ab_line.json" 2> "$OUT/ab_err.log" || { echo "$1: bench.py failed ($?)"; tail -5 "$OUT/ab_err.log"; return 1; }
  python - "$1" "$OUT/ab_line.json" <<'PY' | tee -a "$TAB"
import json, sys
d = json.loads([l for l in open(sys.argv[2]) if l.startswith('{')][-1])
print(f"[{sys.argv[1]:14s}] {d['ms_per_step']:.4f} ms/step  tok/s {d['value']:.0f}  equals_greedy={d['config'].get('lookahead_equals_greedy', d.get('equals_greedy'))}")
PY
}
for v in $(seq "$VISITS"); do
  visit "37=0 visit $v" 0 || exit 1
  for f in $FORMS; do visit "37=$f visit $v" "$f" || exit 1; done
done
[ -n "${NO_PROFILE:-}" ] && exit 0
for f in 0 $FORMS; do
  D=$(mktemp -d)
  LA_DEBUG="37=$f" timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$D" -o run -- python bench.py --gpus 1 --steps 20 --warmup 4 > "$OUT/prof_$f.log" 2>&1 || { echo "rocprofv3 run of 37=$f failed ($?)"; tail -5 "$OUT/prof_$f.log"; exit 1; }
  python - "$f" "$D" <<'PY' | tee -a "$TAB"
import csv, glob, sys
for p in glob.glob(sys.argv[2] + '/**/*kernel_stats.csv', recursive=True):
    print(f'== rocprofv3 --kernel-trace --stats, 37={sys.argv[1]}: kernels above 1 % of the run')
    for r in csv.DictReader(open(p)):
        if float(r['Percentage']) >= 1.0 or 'k_tree_attn1' in r['Name']:
            print(f"{r['Name'][:70]:70s} calls {int(r['Calls']):6d} avg {float(r['AverageNs']) / 1e3:8.2f} us  min {float(r['MinNs']) / 1e3:7.2f}  total {float(r['TotalDurationNs']) / 1e6:9.2f} ms  {float(r['Percentage']):5.1f} %")
PY
  rm -rf "$D"
done

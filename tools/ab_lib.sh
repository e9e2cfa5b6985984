#!/bin/bash
# same-box A/B of two builds of the library, printed to stdout: tools/ab_lib.sh [a b]
# expects medicalsemseg_amd/libmsseg_hip_<a>.so and _<b>.so (default: old new) and selects them with MSSEG_LIB, two alternating
# rounds; "old old" gives the run-to-run spread of one build against itself.  The first failing step ends the script.
set -o pipefail
a=${1:-old}; b=${2:-new}
L=$PWD/medicalsemseg_amd
step() {   # step <label> <time limit> <command ...>: last output line, labelled
  local label=$1 limit=$2; shift 2
  timeout -k 10 $limit "$@" 2>&1 | tail -1 | sed "s/^/$label /" || { echo "$label: failed"; exit 1; }
}
bench_json() {   # bench_json <label> <field> <bench.py arguments ...>
  local label=$1 field=$2; shift 2
  timeout -k 10 300 python bench.py "$@" 2>/dev/null | tail -1 |
    python -c "import json,sys; print('$label', json.loads(sys.stdin.read())['$field'])" || { echo "$label: failed"; exit 1; }
}
for round in 1 2; do
  for v in $a $b; do
    export MSSEG_LIB=$L/libmsseg_hip_$v.so
    id="$v r$round"; [ $a = $b ] && id="$v r$round.$((++n))"
    for w in fwd fwdstats; do step "$id B2" 120 python tools/bench_conv.py $w 32 32 96 20; done
    MSSEG_BENCH_N=8 step "$id B8" 120 python tools/bench_conv.py fwdstats 32 32 96 20
    step "$id B2" 120 python tools/bench_conv.py wgrad 32 32 96 20
    step "$id B2" 120 python tools/bench_conv.py wgrad 64 32 96 20
    timeout -k 10 240 python tools/bench_c48.py 2 2>&1 | grep -E "^ *(96|48)\^3 48-> *(48|96) " | sed "s/^/$id c48 /" || { echo "$id c48: failed"; exit 1; }
    bench_json "$id unet step ms" ms_per_step --no-cpu-baseline --no-sliding-window --steps 30 --warmup 5
    bench_json "$id sliding window vol/s" value --workload sliding_window --no-cpu-baseline --steps 3 --warmup 1
  done
done

#!/bin/bash
# sliding window: K-split of the 24^3 level on / off, three rounds, 5 volumes each, all groups
out=ab/r3c_sw_ab
mkdir -p $out
for r in 1 2 3; do
  MSSEG_NO_KSPLIT_INFER=1 python bench.py --full --workload sliding_window --no-cpu-baseline --steps 5 --all-groups > $out/off_$r.json 2> /dev/null
  python bench.py --full --workload sliding_window --no-cpu-baseline --steps 5 --all-groups > $out/on_$r.json 2> /dev/null
done
python3 - "$out" <<'PY'
import json, sys
out = sys.argv[1]
for k in ("off", "on"):
    vals = [json.load(open(f"{out}/{k}_{r}.json"))["value"] for r in (1, 2, 3)]
    print(k, vals)
for k in ("off", "on"):
    d = json.load(open(f"{out}/{k}_3.json"))
    print(k)
    for g in d["roofline"]["groups"][:14]:
        print(f"  {g['group']:34s} {g['launches_per_step']:7.1f}/vol entry {g['avg_ms']*1e3:7.1f} us tot {g['avg_ms']*g['launches_per_step']:7.1f} ms kernel {g['kernel_avg_ms'] and round(g['kernel_avg_ms']*1e3,1)}")
PY

#!/bin/bash
# A/B timing of library variants built with KZG_BUILD_DIR=ab/<name> (same box, back to back).
#   [OUT=dir] tools/ab_bench.sh name1 name2 ...    -> $OUT/ab_<name>.json (OUT defaults to ab)
# "tree" is the in-tree library.  ab/<name>/env, if there, is sourced for that variant's run (e.g. `export KZG_ACC_WGS_PER_CU=3`);
# a variant with an env file and no library of its own runs the in-tree library under that environment.
OUT=${OUT:-ab}
mkdir -p "$OUT"
for v in "$@"; do
  (
  if [ "$v" = tree ] || { [ -f "ab/$v/env" ] && [ ! -f "ab/$v/libkzg_mi355x.so" ]; }; then unset KZG_MI355X_LIB; else export KZG_MI355X_LIB=$PWD/ab/$v/libkzg_mi355x.so; fi
  if [ -f "ab/$v/env" ]; then . "ab/$v/env"; fi
  python bench.py --full --mode batch --no-cpu-baseline --steps 30 > "$OUT/ab_$v.json" 2> "$OUT/ab_$v.err" || echo "FAILED $v"
  python - "$v" "$OUT" <<'PY'
import json, sys
v, out = sys.argv[1], sys.argv[2]
try:
    d = json.loads(open(f"{out}/ab_{v}.json").read().strip().splitlines()[-1])
    iso = d.get("kernel_ms_per_commit_isolated", {})
    print(f"{v:14s} {d['value']:7.1f} commits/s  acc pipelined {d['kernel_ms_per_commit']['msm_accumulate']:.3f} ms  alone {d['roofline']['isolated']['avg_launch_ms']:.3f} ms  ntt {d['ntt_ms']*1e3:.1f} us  "
          f"alone: p1 {iso.get('msm_partition1', 0):.3f} p2 {iso.get('msm_partition2', 0):.3f} order {iso.get('msm_order', 0):.3f} fin {iso.get('msm_finalize', 0):.3f} red {iso.get('msm_reduce', 0):.3f}  ok {d['verified']['last_step_commit_trapdoor']}")
except Exception as e:
    print(v, "no result", e)
PY
  )
done

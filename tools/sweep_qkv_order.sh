#!/bin/bash
# Sweep of the fused QKV + attention launch's request-order knobs on the flagship
# shape (bench.py's plain run), 3 timed steps a point, one line a point:
#   tools/sweep_qkv_order.sh OUT "kvw=8 QASR_KVW_DELAY=8" "kvw=8,qkv=4 QASR_KVW_DELAY=8 QASR_FUSE_DELAY=4" ...
# Each argument after OUT is a tag followed by the environment of that point
# (QASR_KVW_DELAY, QASR_K_STAGGER, QASR_VT_STAGGER, QASR_FUSE_DELAY, QASR_FUSE_ODELAY;
# "base" alone = the defaults).  Lines go to OUT and to stdout: tag, RTFx, ms a
# step, decode ms a step.  Stops at the first run that fails.
out=$1; shift
mkdir -p "$(dirname "$out")"
for point in "$@"; do
    set -- $point
    tag=$1; shift
    env "$@" timeout -k 10 200 python -u bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-probe > "$out.log" 2>&1 || { tail -5 "$out.log"; exit 1; }
    grep '^{' "$out.log" | tail -1 | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('$tag', d['value'], d['ms_per_step'], d['stage_ms_per_step_rank0']['decode'])" | tee -a "$out"
done

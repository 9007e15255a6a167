# round-3 evidence: full GPU suite, smoke, the bench line of bench.py --full (with the CPU baseline)
export TMPDIR=/tmp
mkdir -p gpurun_out
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 580 --timeout-method thread > gpurun_out/final_t.log 2>&1; rc=$?; tail -3 gpurun_out/final_t.log; [ $rc -ne 0 ] && { grep -E "FAIL|Error" gpurun_out/final_t.log | head; exit $rc; }
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > gpurun_out/final_smoke.log 2>&1 || { tail -5 gpurun_out/final_smoke.log; exit 1; }
tail -1 gpurun_out/final_smoke.log
BLOG=$(mktemp)   # bench.py --full: the line with cpu_baseline, roofline_other and utterance_set
timeout -k 10 600 python -u bench.py --full > "$BLOG" 2>&1 || { tail -5 "$BLOG"; exit 1; }
grep '^{' "$BLOG" | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['stage_ms_per_step_rank0'], d['cpu_baseline'], [(x['kernel'][:30], x['avg_launch_us'], x['frac']) for x in [d['roofline']]+d['roofline_other']])"

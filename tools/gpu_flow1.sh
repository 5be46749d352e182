#!/bin/bash
out=gpurun_out/flow1; mkdir -p $out; export TMPDIR=/tmp
timeout -k 10 240 python tools/flow_check.py > $out/check.txt 2>&1; echo "check rc=$?" | tee $out/steps.log; tail -12 $out/check.txt
[ "$(tail -1 $out/steps.log)" = "check rc=0" ] || exit 1
timeout -k 10 120 python tools/flow_check.py stamps > $out/stamps.txt 2>&1; echo "stamps rc=$?" | tee -a $out/steps.log; tail -14 $out/stamps.txt
for dbg in 0 2048 1024; do
timeout -k 10 200 python bench.py --full --steps 60 --warmup 5 --no-cpu-baseline --repeats 3 --debug $dbg 2>/dev/null | python3 -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('debug $dbg', round(d['value'],1), round(d['ms_per_step']*1e3,2), {k: round(v*1e3,1) for k,v in d['kernel_ms'].items()}, d['rmse_px'])" | tee -a $out/bench.txt
done

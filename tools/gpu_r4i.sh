#!/bin/bash
out=${1:-r4i}; mkdir -p "$out"
for rep in 1 2; do for g in 4 2 8 16; do
  SFM_REDUCE_SLICES=$g SFM_HIP_LIBRARY=$PWD/${AB_DIR:?folder of the A/B builds}/slices.so timeout -k 10 200 python bench.py --full --steps 60 --warmup 5 --no-cpu-baseline --repeats 3 2>/dev/null | python3 -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('slices $g', round(d['value'],1), round(d['ms_per_step']*1e3,2), {k: round(v*1e3,1) for k,v in d['kernel_ms'].items()})" | tee -a "$out/ab_reduce_slices.txt"
done; done

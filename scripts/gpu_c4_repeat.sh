#!/bin/bash
# three plain configs[4] bench runs.  usage: scripts/gpu_c4_repeat.sh [outdir]
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$ROOT/bench_out}
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT
for i in 1 2 3; do
timeout -k 10 300 python -u bench.py --workload config4 > $OUT/c4_$i.json 2> $OUT/c4_$i.log || exit 1
python3 -c "import json; d=json.load(open('$OUT/c4_$i.json')); print('config4', d['value'], d['ms_per_step'])"
done

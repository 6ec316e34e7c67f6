#!/bin/bash
# configs[3] bench at 2 / 3 / 4 / 6 contexts per GPU (plain runs), alternated twice.  usage: scripts/gpu_c3_ctx.sh [outdir]
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$ROOT/bench_out}
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT
for r in 1 2; do for g in 2 3 4 6; do
  timeout -k 10 300 python -u bench.py --workload config3 --steps 60 --contexts $g > $OUT/c3ctx_${g}_$r.json 2> $OUT/c3ctx_${g}_$r.log || exit 1
  python3 -c "import json; d=json.load(open('$OUT/c3ctx_${g}_$r.json')); print('contexts', $g, d['value'], d['ms_per_step'])"
done; done

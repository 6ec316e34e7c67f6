#!/bin/bash
# configs[4] bench line (one GPU, oracle-verified: --full) and two plain repeats.  usage: scripts/gpu_c4.sh tag [outdir]
TAG=${1:-c4}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${2:-$ROOT/bench_out}
cd $ROOT && export TMPDIR=/tmp && mkdir -p $OUT
timeout -k 10 400 python -u bench.py --workload config4 --full > $OUT/bench_c4_$TAG.json 2> $OUT/bench_c4_$TAG.log || { tail -20 $OUT/bench_c4_$TAG.log; exit 1; }
python3 -c "import json; d=json.load(open('$OUT/bench_c4_$TAG.json')); print('config4', d['value'], d['ms_per_step'], d.get('oracle_verified_sources'), d['config']['contexts_per_gpu'])"
for i in 1 2; do
timeout -k 10 300 python -u bench.py --workload config4 > $OUT/c4r_$i.json 2> $OUT/c4r_$i.log || exit 1
python3 -c "import json; d=json.load(open('$OUT/c4r_$i.json')); print('config4', d['value'], d['ms_per_step'])"
done

#!/bin/bash
# usage (on the GPU box): bash tools/bench_stats.sh [rows] -- bench.py JSON line + rocprofv3 kernel stats of the same command
# Writes bench_stats.json and bench_kernel_stats.csv to $OUT_DIR (default: bench_out/ in the repository).
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${OUT_DIR:-$R/bench_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/bs
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/bs -o bs -- python3 $R/bench.py --full --no-cpu-baseline --no-lut --no-opt125m --no-llama --no-stress --no-tiny > $O/bench_stats.json 2>/tmp/bs.err || { tail -5 /tmp/bs.err; exit 1; }
cp "$(find /tmp/bs -name 'bs_kernel_stats.csv' | head -1)" $O/bench_kernel_stats.csv
python3 $R/tools/top_kernels.py $O/bench_kernel_stats.csv ${1:-24}
tail -1 $O/bench_stats.json | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['kernels'].get('t_prepare_kernels'))"

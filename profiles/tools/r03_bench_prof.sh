#!/bin/bash
# Round-3 evidence for the bench line: (1) the default run with --full, (2) the
# command under rocprofv3 --kernel-trace --stats restricted to the timed
# region, (3) HBM traffic of the bound-evaluation kernels (bench.py
# --pmc-traffic: FETCH_SIZE / WRITE_SIZE in separate child passes).
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$PWD}
OUT=$R/gpurun_out/r03
mkdir -p $OUT
cd $R
python bench.py --full > $OUT/bench_r03.json 2> $OUT/bench_r03.err
tail -c 600 $OUT/bench_r03.json
cd /tmp
rm -rf /tmp/r03_bench
timeout 600 rocprofv3 --kernel-trace --stats --marker-trace --selected-regions --output-format csv -d /tmp/r03_bench -o bench -- python $R/bench.py --no-cpu-baseline > /tmp/bench_prof.log 2>&1
grep '^{"metric"' /tmp/bench_prof.log | tail -1 > $OUT/bench_profiled.json
find /tmp/r03_bench -name '*kernel_stats.csv' | head -1 | xargs -I{} cp {} $OUT/bench_kernel_stats.csv
head -8 $OUT/bench_kernel_stats.csv | cut -c1-200
cd $R
timeout 1500 python bench.py --no-cpu-baseline --pmc-traffic > $OUT/bench_pmc_traffic.json 2> $OUT/bench_pmc.err
python - <<'PY'
import json, os
p = os.path.join(os.environ.get('GRAFT_REPO_ROOT', '.'), 'gpurun_out/r03/bench_pmc_traffic.json')
try:
    r = json.load(open(p))['roofline']
    print('traffic', r['traffic'], 'algorithmic', r['algorithmic_bytes_per_launch'], r['traffic_source'])
except Exception as e:
    print('pmc failed', e)
PY

#!/bin/bash
# bench.py --full (headline + moving camera + configs 2/4/5 + CPU baseline), timed; counters the profiler offers
# usage: bash tools/gpu_bench_full.sh OUTPUT_DIR     (relative to the repo root)
O=${1:?usage: bash tools/gpu_bench_full.sh OUTPUT_DIR}
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
mkdir -p $O
( time timeout -k 10 900 python bench.py --full > $O/default.json 2> $O/default.err ) 2> $O/default.time
rc=$?
tail -3 $O/default.err; cat $O/default.time
python - "$O" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1] + '/default.json').read().strip().splitlines()[-1])
print('headline', d['value']/1e9, 'G', d['ms_per_step'], 'ms verified', d['verified'])
for k,v in (d.get('configs') or {}).items():
    print(k, v if not isinstance(v,dict) else {kk:v[kk] for kk in ('ms_per_frame','path_rays_per_s','verified','kernel','scene_setup_s') if kk in v})
print('cpu', d.get('cpu_baseline'))
PY
timeout 120 rocprofv3 -L > $O/counters.txt 2>&1; grep -i "f64\|F32\|FLOP\|SQ_INSTS_VALU" $O/counters.txt | head -40
exit $rc

#!/bin/bash
# The round's evidence set, on an MI355X: rocprofv3 kernel trace (overlapped + serialised) and PMC passes per BASELINE config
# (tools/profile_bench.sh -> $PS_PROFILE_OUT/prof_<cfg>/, default profile_out/), the streaming kernel's profile (PS_DAAT=0), and
# the bench lines (bench.py --full: roofline, CPU baseline and the other legs).
#   usage: tools/round_profiles.sh <round tag, e.g. r06> <git head>
# Afterwards, here: python tools/collect_profile.py <tag> C2 C3 C4 C5 C2stream; copy $PS_PROFILE_OUT/<tag>final/bench_*.json into profiles/.
TAG=$1; HEAD=$2
R=${GRAFT_REPO_ROOT:-$PWD}
cd $R
export PS_PROFILE_OUT=${PS_PROFILE_OUT:-$R/profile_out}
OUT=$PS_PROFILE_OUT
mkdir -p $OUT
for C in C2 C3 C5 C4; do
  bash tools/profile_bench.sh $C $HEAD --config $C > $OUT/prof_$C.log 2>&1
done
PS_DAAT=0 bash tools/profile_bench.sh C2stream $HEAD --config C2 > $OUT/prof_C2stream.log 2>&1
mkdir -p $OUT/${TAG}final
python bench.py --full --gpus 1 --steps 25 --warmup 5 > $OUT/${TAG}final/bench_C2_short_run.json 2> $OUT/${TAG}final/bench_C2_short_run.err
for C in C2 C3 C5 C1 C4; do
  python bench.py --full --config $C --steps 100 --warmup 10 > $OUT/${TAG}final/bench_$C.json 2> $OUT/${TAG}final/bench_$C.err
done
python - <<PY
import json,glob
for f in sorted(glob.glob('$OUT/${TAG}final/bench_*.json')):
    try:
        d=json.loads(open(f).read().strip().splitlines()[-1]); r=d['roofline']
        cb=d.get('cpu_baseline') or {}
        print(f.split('/')[-1], round(d['value']), round(d['ms_per_step'],4), r['kernel'], 'avg', round(r['kernel_avg_ms'],4), 'busy', round(r.get('kernel_busy_avg_ms',0),4), 'serial', round(r.get('kernel_serial_avg_ms') or 0,4),
              'frac', round(r['frac'],3), 'frac_serial', round(r.get('frac_serial') or 0,3), 'cpu', cb.get('value'), (cb.get('flat') or {}).get('value'), (cb.get('all_cores') or {}).get('value'), 'mism', cb.get('gpu_topk_mismatches_vs_oracle'),
              'upd', (d.get('live_index_updates') or {}).get('ratio'))
    except Exception as e:
        print(f,'ERR',e)
PY

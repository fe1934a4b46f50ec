#!/bin/bash
# the data-parallel step on a world of ONE rank over the real RCCL backend vs the plain single-process step (same box)
#   bash tools/exp/dp_single.sh OUT_DIR
O=${1:?usage: dp_single.sh OUT_DIR}
mkdir -p $O
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-psnr > $O/plain.json 2> $O/plain.err
PERF_DP_SINGLE_RANK=1 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-psnr > $O/rccl1.json 2> $O/rccl1.err
PERF_DP_SINGLE_RANK=1 PERF_DP_GRAPH=0 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-psnr > $O/rccl1_eager.json 2> $O/rccl1_eager.err
DP1_OUT=$O python - <<'PY'
import json, os
o = os.environ['DP1_OUT']
for f in ('plain','rccl1','rccl1_eager'):
    try:
        d=[json.loads(l) for l in open(f"{o}/{f}.json") if l.startswith("{")][-1]
        print(f, d['ms_per_step'], d['value'], d.get('launch'), (d.get('strict_two_evaluations') or {}).get('ms_per_step'), (d.get('sustained') or {}).get('ms_per_step'))
    except Exception as e:
        print(f, 'FAILED', e); print(open(f'{o}/{f}.err').read()[-1500:])
PY

#!/bin/bash
# pipelined K3: half-row tail kernel (8 lanes per channel) against the default, over priorities
# (--full: the line's kernels_ms_isolated; --no-extra-legs keeps the run to the one configuration)
ERR=$(mktemp)
for tv in 16r 8r; do for pr in ${PRIOS:-2,2 2,3 1,2 0,3 2,1}; do
RDSP_TAIL_VARIANT=$tv RDSP_PRIO=$pr python bench.py --full --config ${K:-K3} --steps ${STEPS:-100} --warmup ${WARMUP:-20} --no-cpu-baseline --no-host-io --no-extra-legs 2>$ERR | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('tail $tv prio $pr ms/step %.3f'%d['ms_per_step'], {k:round(v,3) for k,v in d['kernels_ms_per_step'].items()}, {k:round(v,3) for k,v in (d['kernels_ms_isolated'] or {}).items()})" || tail -3 $ERR
done; done
rm -f $ERR

#!/bin/bash
# Round 5, after the tail kernels' load batching: the block cap of the tail's big-grid kernels and the worker count on the
# headline pages and the dense ones, one box, 40 timed steps each.  Each line = pages/s, ms per step, cores.  (The run of a
# variant library with eight groups in flight in the block-per-window kernels went with those kernels; its
# result is in DESIGN 4.12.)
cd "${GRAFT_REPO_ROOT:-$(pwd)}" || exit 1
run() { echo "$CTD_TUNING $*: $(python bench.py --no-cpu-baseline --no-extras --steps 40 --warmup 5 "$@" 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().splitlines()[-1]); print(d['value'], d['ms_per_step'], d['config']['host_cpu_cores_used'])")"; }
run
CTD_TUNING=tail_max_blocks=512 run
CTD_TUNING=tail_max_blocks=768 run
CTD_TUNING=tail_max_blocks=2048 run
run --workers 3
run --dense-blocks
CTD_TUNING=tail_max_blocks=512 run --dense-blocks
CTD_TUNING=tail_max_blocks=2048 run --dense-blocks
run

#!/bin/bash
# usage: [WL=workload] [ROUNDS=2] [STEPS=3] [WARMUP=1] [READS=n] tools/ab_builds.sh name1 name2 ...
# A/B of libsfa_<name>.so builds on bench.py, interleaved rounds in one call.  Every bench run has its own time limit and the
# runs are chained: the first one that fails, faults or times out ends the script.
# One line per run: workload, build, reads/s, ms_per_step, kernel_ms_per_step, trace_kernel_ms_per_step
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
WL=${WL:-ncov_r9_dna_q250}
ROUNDS=${ROUNDS:-2}
STEPS=${STEPS:-3}
WARMUP=${WARMUP:-1}
for round in $(seq 1 "$ROUNDS"); do
for n in "$@"; do
  SFA_LIB=$ROOT/sigfish_amd/lib/libsfa_$n.so timeout -k 10 200 python "$ROOT/bench.py" --workload "$WL" ${READS:+--reads $READS} --steps "$STEPS" --warmup "$WARMUP" --no-cpu-baseline --no-e2e 2>/dev/null \
    | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$WL', '$n', d['value'], d['ms_per_step'], d['roofline']['kernel_ms_per_step'], d['roofline']['trace_kernel_ms_per_step'])" \
    || exit 1
done; done

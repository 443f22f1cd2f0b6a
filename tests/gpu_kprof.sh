#!/bin/bash
# usage: tests/gpu_kprof.sh <tag> [pattern] [outdir]   — kernel-trace of bench.py (20 steps), prints the per-kernel summary
# per registration of the trace (settle and warm-up included); the trace stays under outdir (default prof_out/)
tag=${1:-x}; pat=${2:-}
R=$(cd "$(dirname "$0")/.." && pwd); O=$(mkdir -p "${3:-$R/prof_out}" && cd "${3:-$R/prof_out}" && pwd)
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace -d $O/prof_$tag -o $tag -- python $R/bench.py --steps 20 --warmup 5 > $O/prof_$tag.log 2>&1 || exit $?
python $R/profiles/summarize_rocpd.py $O/prof_$tag/${tag}_results.db auto | grep -i "registrations\|$pat" | head -40

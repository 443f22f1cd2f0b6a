#!/bin/bash
# usage: tests/gpu_profile_all.sh <tag> [outdir] — bench JSON (--full), kernel trace, and the two PMC passes (FETCH_SIZE /
# WRITE_SIZE) of bench.py's headline loop; everything under outdir (default prof_out/).  Every GPU step runs under its own
# time limit, and the first one that does not exit cleanly ends the script.
tag=${1:-x}
R=$(cd "$(dirname "$0")/.." && pwd); O=$(mkdir -p "${2:-$R/prof_out}" && cd "${2:-$R/prof_out}" && pwd)
step() { "$@" || { echo "stopped: exit status $? of: $*" >&2; exit 1; }; }
step timeout -k 10 900 python $R/bench.py --full > $O/bench_$tag.json 2> $O/bench_$tag.err
cd /tmp && export TMPDIR=/tmp
step timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_$tag -o $tag -- python $R/bench.py --steps 20 --warmup 5 > $O/prof_$tag.log 2>&1
step timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $O/pmc_fetch_$tag -o fetch -- python $R/bench.py --steps 8 --warmup 2 > $O/pmc_fetch_$tag.log 2>&1
step timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $O/pmc_write_$tag -o write -- python $R/bench.py --steps 8 --warmup 2 > $O/pmc_write_$tag.log 2>&1
ls $O/prof_$tag $O/pmc_fetch_$tag $O/pmc_write_$tag
tail -c 600 $O/bench_$tag.json

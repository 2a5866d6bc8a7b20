#!/bin/bash
# Round-end evidence (run on the GPU box): the full bench line (bench.py --full), the same command under
# rocprofv3 --kernel-trace --stats, summaries under OUTDIR/TAG (copy the ones to keep into profiles/).
#   tools/profile_round.sh TAG OUTDIR
R=${GRAFT_REPO_ROOT:-/root/repo}
TAG=${1:-r01}
O=$(realpath -m "${2:?usage: tools/profile_round.sh TAG OUTDIR}")/$TAG
mkdir -p $O
cd $R && python bench.py --full > $O/bench.json 2> $O/bench.err
tail -1 $O/bench.json | cut -c1-400
cd /tmp && export TMPDIR=/tmp
timeout 900 rocprofv3 --kernel-trace --stats -d $O/prof -o trace -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-single > $O/bench_under_rocprof.json 2> $O/rocprof.err
db=$(find $O/prof -name "*.db" | head -1)
if [ -n "$db" ]; then
  python $R/tools/rocpd_stats.py $db > $O/kernel_stats.txt
  python $R/tools/rocpd_stats.py $db --by-grid > $O/kernel_stats_by_grid.txt
  head -14 $O/kernel_stats.txt
  rm -rf $O/prof
else
  tail -5 $O/rocprof.err
fi

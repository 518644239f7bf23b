#!/bin/bash
# rocprofv3 kernel-trace summary of a short bench run: scripts/prof.sh <tag> [bench args]
set -u
tag=$1; shift
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
o=${FS2_PROF_OUT:-prof_out}; mkdir -p $o
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $o/prof_$tag -o $tag --output-format csv \
  -- python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-traffic "$@" > $o/prof_$tag.log 2>&1
rc=$?
tail -1 $o/prof_$tag.log | cut -c1-300
exit $rc

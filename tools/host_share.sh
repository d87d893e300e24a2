#!/bin/bash
# The host's share of a Gibbs iteration ("The host's share"): a parent build and this tree alternating in
# one job, so that both see the same machine.  Per pair: bench.py defaults at c4 (the headline), then c4, c3 and c2 with
# HGIBBS_TIMING=1 (the per-line breakdown on stderr); two --dump-outputs runs of the parent and one of this tree, compared;
# one rocprofv3 kernel + memory-copy trace of each (no counters); the shuffle's host-only timing.
# Every GPU step has its own limit and the job stops at the first step that fails.
# usage (repository root, both trees built): bash tools/host_share.sh PARENT_TREE [OUT_DIR] [PAIRS]
set -o pipefail
PARENT=${1:?usage: tools/host_share.sh PARENT_TREE [OUT_DIR] [PAIRS]}
O=${2:-build/host_share}
PAIRS=${3:-5}
HERE=$(dirname "$0")
mkdir -p $O
export TMPDIR=/tmp
run () { # tag tree config index timing
  local TAG=$1 TREE=$2 C=$3 I=$4 T=$5
  if [ "$T" = 1 ]; then
    HGIBBS_TIMING=1 timeout -k 10 240 python3 $TREE/bench.py --config $C --no-cpu-baseline --no-anatomy > $O/${TAG}_${C}_t_$I.json 2> $O/${TAG}_${C}_t_$I.err
  else
    timeout -k 10 240 python3 $TREE/bench.py --config $C --no-cpu-baseline --no-anatomy > $O/${TAG}_${C}_$I.json 2> $O/${TAG}_${C}_$I.err
  fi
}
for I in $(seq 1 $PAIRS); do
  run parent $PARENT c4 $I 0 || { echo "parent c4 $I failed"; tail -5 $O/parent_c4_$I.err; exit 1; }
  run result . c4 $I 0 || { echo "result c4 $I failed"; tail -5 $O/result_c4_$I.err; exit 1; }
done
for C in c4 c3 c2; do
  for I in $(seq 1 $PAIRS); do
    run parent $PARENT $C $I 1 || { echo "parent $C $I failed"; tail -5 $O/parent_${C}_t_$I.err; exit 1; }
    run result . $C $I 1 || { echo "result $C $I failed"; tail -5 $O/result_${C}_t_$I.err; exit 1; }
  done
done
# outputs: the parent twice (its own run-to-run spread), this tree once
timeout -k 10 240 python3 $PARENT/bench.py --no-cpu-baseline --no-anatomy --dump-outputs $O/dump_parent_a > /dev/null 2> $O/dump_parent_a.err || { echo "dump a failed"; exit 1; }
timeout -k 10 240 python3 $PARENT/bench.py --no-cpu-baseline --no-anatomy --dump-outputs $O/dump_parent_b > /dev/null 2> $O/dump_parent_b.err || { echo "dump b failed"; exit 1; }
timeout -k 10 240 python3 bench.py --no-cpu-baseline --no-anatomy --dump-outputs $O/dump_result > /dev/null 2> $O/dump_result.err || { echo "dump of this tree failed"; tail -5 $O/dump_result.err; exit 1; }
python3 $HERE/cmp_dumps.py $O/dump_parent_a $O/dump_parent_b $O/dump_result | tee $O/host_share_dumps.txt
rm -rf $O/dump_parent_a $O/dump_parent_b $O/dump_result
for TAG in parent result; do
  TREE=.; [ $TAG = parent ] && TREE=$PARENT
  timeout -k 10 400 rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d $O/kt_$TAG -o kt -- python3 $TREE/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-anatomy > $O/host_share_${TAG}_c4_bench_under_rocprof.json 2> $O/kt_$TAG.err || { echo "rocprofv3 ($TAG) failed: $?"; tail -20 $O/kt_$TAG.err; exit 1; }
  for f in $(find $O/kt_$TAG -name '*kernel_stats.csv' -o -name '*memory_copy_stats.csv'); do cp $f $O/host_share_${TAG}_c4_$(basename $f | sed 's/^kt_//'); done
  python3 $HERE/trace_gaps.py $O/kt_$TAG > $O/host_share_${TAG}_c4_trace_gaps.txt
  rm -rf $O/kt_$TAG
done
if [ -x $HERE/shuffle_bench ]; then timeout -k 10 200 $HERE/shuffle_bench 1000000 7 | tee $O/host_share_shuffle_bench.txt; fi
python3 $HERE/host_share_fold.py $O $PAIRS | tee $O/host_share_runs.txt

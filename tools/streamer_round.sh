#!/bin/bash
# The streaming workgroups' instructions per round: a parent build and this tree alternating in one job, so
# that both see the same machine.  bench.py defaults at c4 (PAIRS runs each), two runs each of c3 and c2; `--config c2 --opt
# early_advance=0 --dump-outputs` twice on the parent and once on this tree, compared by cmp_dumps.py (no timing-dependent message:
# the chain must be bit-identical); the stage anatomy of both builds, twice; per tree one rocprofv3 kernel trace and, in a run of
# its own, the SQ counters (SQ_INSTS_VALU per sweep) and tools/res_anatomy.py's lines on the chain's record stage.  Every GPU step has its own limit and the job stops at the first that fails.
# The files that are kept are named PREFIX_* (default streamer_round; the decider's round of section 8 used decider_round).
# usage (repository root, both trees built): bash tools/streamer_round.sh PARENT_TREE [OUT_DIR] [PAIRS] [PREFIX]
set -o pipefail
PARENT=$(cd "${1:?usage: tools/streamer_round.sh PARENT_TREE [OUT_DIR] [PAIRS] [PREFIX]}" && pwd)
ROOT=$(pwd)
O=${2:-build/streamer_round}
PAIRS=${3:-5}
P=${4:-streamer_round}
mkdir -p $O && O=$(cd $O && pwd)
export TMPDIR=/tmp
stop () { echo "STOP: $1 (exit status $2)"; exit 1; }
tree_of () { [ $1 = parent ] && echo $PARENT || echo $ROOT; }
run () { # tag config index
  ( cd $(tree_of $1) && timeout -k 10 240 python3 bench.py --config $2 --no-cpu-baseline --no-anatomy > $O/$1_$2_$3.json 2> $O/$1_$2_$3.err )
}
for I in $(seq 1 $PAIRS); do
  for TAG in parent result; do run $TAG c4 $I || stop "$TAG c4 $I" $?; done
done
for C in c3 c2; do
  for I in 1 2; do
    for TAG in parent result; do run $TAG $C $I || stop "$TAG $C $I" $?; done
  done
done
dump () { # tag suffix
  ( cd $(tree_of $1) && timeout -k 10 240 python3 bench.py --config c2 --opt early_advance=0 --no-cpu-baseline --no-anatomy --dump-outputs $O/dump_$1$2 > /dev/null 2> $O/dump_$1$2.err )
}
dump parent _a || stop "dump parent a" $?
dump parent _b || stop "dump parent b" $?
dump result "" || stop "dump result" $?
python3 $ROOT/tools/cmp_dumps.py $O/dump_parent_a $O/dump_parent_b $O/dump_result | tee $O/${P}_dumps.txt
rm -rf $O/dump_parent_a $O/dump_parent_b $O/dump_result
for I in 1 2; do
  for TAG in parent result; do
    ( cd $(tree_of $TAG) && timeout -k 10 240 python3 bench.py --no-cpu-baseline > $O/${TAG}_c4_anatomy_$I.json 2> $O/${TAG}_c4_anatomy_$I.err ) || stop "$TAG anatomy $I" $?
  done
done
for TAG in parent result; do
  cd $(tree_of $TAG)
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/kt_$TAG -o kt -- python3 bench.py --steps 3 --warmup 2 --no-cpu-baseline --no-anatomy > $O/${TAG}_c4_bench_under_rocprof.json 2> $O/kt_$TAG.err || stop "rocprofv3 kernel trace ($TAG)" $?
  DB=$(ls $O/kt_$TAG/*results.db $O/kt_$TAG/*/*results.db 2>/dev/null | head -1)
  python3 $ROOT/tools/rocpd_stats.py $DB $O/${P}_${TAG}_c4_kernel_stats.csv k_sweep_limb 3 > $O/${P}_${TAG}_c4_kernel_timed_region.txt || stop "rocpd_stats ($TAG)" $?
  rm -rf $O/kt_$TAG
  timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAVES GRBM_GUI_ACTIVE -d $O/pmc_$TAG -o p -- python3 bench.py --steps 3 --warmup 2 --no-cpu-baseline --no-anatomy > $O/pmc_$TAG.json 2> $O/pmc_$TAG.err || stop "rocprofv3 counters ($TAG)" $?
  DB=$(ls $O/pmc_$TAG/*results.db $O/pmc_$TAG/*/*results.db 2>/dev/null | head -1)
  python3 $ROOT/tools/rocpd_pmc.py $DB k_sweep_limb 3 > $O/${P}_${TAG}_c4_pmc_SQ1.txt || stop "rocpd_pmc ($TAG)" $?
  rm -rf $O/pmc_$TAG
  # the chain's record stage ("absorb"), which bench.py's anatomy does not print, and the Gram words' way to the walker
  timeout -k 10 300 python3 tools/res_anatomy.py 500000 1000000 4 > $O/${TAG}_c4_res_anatomy_full.txt 2> $O/${TAG}_c4_res_anatomy.err || stop "res_anatomy ($TAG)" $?
  grep -E "^(per message with an update|percentiles of message in flight|walker 2, per round)" $O/${TAG}_c4_res_anatomy_full.txt > $O/${P}_${TAG}_c4_res_anatomy.txt || stop "res_anatomy lines ($TAG)" $?
  cd $ROOT
done
python3 $ROOT/tools/streamer_round_fold.py $O | tee $O/${P}_runs.txt

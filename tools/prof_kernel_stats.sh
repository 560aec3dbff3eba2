set -x
O=${PROF_OUT:-prof_out/kernel_stats}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_stage -o stage -- python3 tools/stage_bench.py --size 1080p --reps 4 --matchers > $O/stage_bench.json 2> $O/stage.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_bench -o bench -- python3 bench.py --full --steps 200 --warmup 10 --cpu-rows 0 > $O/bench_profiled.json 2> $O/bench.err
find $O -name "*kernel_stats*" | head; ls $O/prof_stage | head

# bench evidence run: default bench line (CPU baseline, scaling reference),
# rocprofv3 kernel trace + stats of the same command, and two PMC passes
# (FETCH_SIZE, WRITE_SIZE; separate runs) targeting the dominant kernel.
# usage: tools/gpu_bench.sh TAG [STEPS]
set -o pipefail
OUT=${OUT:-bench_out}   # where the results go (relative to the repository root)
export TMPDIR=/tmp
tag=$1
steps=${2:-50}
R=$GRAFT_REPO_ROOT
mkdir -p $R/$OUT
cd $R
timeout -k 10 400 python -u bench.py --full --steps $steps --warmup 10 > $OUT/bench_$tag.json 2> $OUT/bench_$tag.err || { echo BENCH_FAIL; tail -20 $OUT/bench_$tag.err; exit 1; }
cat $OUT/bench_$tag.json
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/prof_$tag -o run -- python3 $R/bench.py --full --steps $steps --warmup 10 --no-cpu-baseline --no-scaling-reference --no-real-data > $R/$OUT/prof_bench_$tag.json 2> $R/$OUT/prof_$tag.err || { echo PROF_FAIL; tail -20 $R/$OUT/prof_$tag.err; exit 1; }
timeout -s KILL 150 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $R/$OUT/pmcf_$tag -o run -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-scaling-reference --no-real-data --pmc-target 20 > $R/$OUT/pmcf_bench_$tag.json 2> $R/$OUT/pmcf_$tag.err || { echo PMC_FETCH_FAIL; tail -20 $R/$OUT/pmcf_$tag.err; exit 1; }
timeout -s KILL 150 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $R/$OUT/pmcw_$tag -o run -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-scaling-reference --no-real-data --pmc-target 20 > $R/$OUT/pmcw_bench_$tag.json 2> $R/$OUT/pmcw_$tag.err || { echo PMC_WRITE_FAIL; tail -20 $R/$OUT/pmcw_$tag.err; exit 1; }
echo done

# usage: [BENCH_ARGS="--config 4"] [PMC_STEPS="--steps 20 --warmup 3"] pmc_pass.sh OUTDIR "COUNTER COUNTER ..." ["COUNTERS of a second pass" ...] — separate rocprofv3 --pmc passes of the bench workload
# PMC_STEPS: the frames of a pass (default --steps 2 --warmup 1).  Where frames of a run differ — the node pipeline's first frame per renderer builds the
# level-0 stage, the others replay it — a pass needs enough of them for the per-frame mean to be the steady state's.
set -e -o pipefail
R=$GRAFT_REPO_ROOT
OUT=$R/$1; shift
cd /tmp && export TMPDIR=/tmp
mkdir -p $OUT
for c in "$@"; do
  d=$OUT/$(echo $c | tr ' ' '_' | cut -c1-48)
  timeout -k 10 200 rocprofv3 --pmc $c --output-format csv -d $d -- python3 $R/bench.py $BENCH_ARGS ${PMC_STEPS:---steps 2 --warmup 1} --no-cpu-baseline > $d.log 2>&1 || { echo "pass $c failed"; tail -5 $d.log; exit 1; }
  echo "pass $c done"
done
python3 $R/tools/pmc_summary.py $OUT > $OUT/summary.txt

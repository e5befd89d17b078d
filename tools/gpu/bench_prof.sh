# bench (--full) + rocprofv3 kernel-trace summary, from the repository root; results go to $OUT
set -o pipefail
export TMPDIR=/tmp
TAG=${TAG:-r01}
STEPS=${STEPS:-20}
O=${OUT:-bench_out}
mkdir -p $O
timeout -k 10 400 python bench.py --full --steps $STEPS --warmup 3 > $O/bench_$TAG.json 2> $O/bench_$TAG.err
rc=$?; echo "bench rc=$rc"; cat $O/bench_$TAG.json; tail -5 $O/bench_$TAG.err
[ $rc -eq 0 ] || exit $rc
if [ -n "$PROF" ]; then
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -o run -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > $O/prof_$TAG.log 2>&1
  rc=$?; echo "rocprof rc=$rc"; tail -3 $O/prof_$TAG.log
  find $O/prof_$TAG -name "*stats*.csv" | head
fi
exit $rc

# Full GPU pass (used via gpurun): GPU tests, PMC traffic of the linearize, bench, rocprof kernel stats.
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${DDLO_OUT:-bench_out}   # where the logs, traces and result lines go
mkdir -p $O
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $O/pytest_gpu.log 2>&1 || { echo PYTEST_FAIL; tail -30 $O/pytest_gpu.log; exit 1; }
tail -3 $O/pytest_gpu.log
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -s KILL 150 rocprofv3 --pmc $c --output-format csv -d $O/pmc_t_$c -o run -- python3 bench.py --full --no-cpu --no-sharded --no-batch --no-odom --no-gn --no-seg --steps 5 --warmup 1 > $O/pmc_t_$c.log 2>&1 || { echo "PMC pass $c failed"; tail -5 $O/pmc_t_$c.log; exit 1; }
done
python3 tools/pmc_traffic.py $O/pmc_t_FETCH_SIZE/run_counter_collection.csv $O/pmc_t_WRITE_SIZE/run_counter_collection.csv $O/traffic.json
DDLO_TRAFFIC_JSON=$O/traffic.json timeout -k 10 600 python -u bench.py --full > $O/bench.json 2> $O/bench.err || { echo BENCH_FAIL; tail -20 $O/bench.err; exit 1; }
cat $O/bench.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_bench -o run -- python3 bench.py --full --no-cpu --no-sharded --no-batch --no-odom --no-gn --no-seg --steps 20 > $O/prof_bench.log 2>&1 || { echo PROF_FAIL; tail -20 $O/prof_bench.log; exit 1; }
python3 tools/profile_summary.py $O/prof_bench run > $O/prof_bench.md
echo ALL_OK

# bench.py's batched leg (after the headline) at 3 / 4 / 6 workers (used via gpurun)
cd $GRAFT_REPO_ROOT
O=${DDLO_OUT:-bench_out}/benchstreams   # where the result lines go
mkdir -p $O
for ns in 3 4 6; do
  timeout -k 10 300 python -u bench.py --full --no-cpu --no-sharded --no-gn --no-odom --no-seg --steps 10 --batch-streams $ns > $O/b$ns.json 2> $O/b$ns.err || { tail -20 $O/b$ns.err; exit 1; }
  python3 -c "import json; b = json.load(open('$O/b$ns.json'))['batched_s2s']; print('streams $ns', b['ms_per_pair'], b['ms_per_pair_morton_tie_order'])"
done

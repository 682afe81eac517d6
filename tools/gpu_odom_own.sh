# odometry driver: partial tree beside the covariance kernel vs gated on its own stream (used via gpurun)
cd $GRAFT_REPO_ROOT
O=${DDLO_OUT:-bench_out}/odomown   # where the result lines go
mkdir -p $O
for os in 0 1; do
  DDLO_NF_OWN_STREAM=$os timeout -k 10 300 python -u bench.py --full --no-cpu --no-sharded --no-gn --no-seg --no-batch --steps 10 > $O/b$os.json 2> $O/b$os.err || { tail -20 $O/b$os.err; exit 1; }
  python3 -c "import json; d = json.load(open('$O/b$os.json')); print('own stream $os', d['odometry']['ms_per_frame'], d['odometry']['ms_per_frame_morton_tie_order'])"
done
for os in 0 1; do
  DDLO_NF_OWN_STREAM=$os DDLO_ODOM_TIMING=1 timeout -k 10 300 python -u bench.py --full --no-cpu --no-sharded --no-gn --no-seg --no-batch --steps 10 > $O/t$os.json 2> $O/t$os.err || { tail -20 $O/t$os.err; exit 1; }
  echo "own stream $os"; grep "odom timing" $O/t$os.err | tail -2
done

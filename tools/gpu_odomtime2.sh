# odometry per-phase wall times: lazy search vs whole tree (used via gpurun)
cd $GRAFT_REPO_ROOT
O=${DDLO_OUT:-bench_out}/odomtime   # where the result lines go
mkdir -p $O
for lz in 1 0; do
  DDLO_TIE_LAZY=$lz DDLO_ODOM_TIMING=1 timeout -k 10 300 python -u bench.py --full --no-cpu --no-sharded --no-gn --no-seg --no-batch --steps 10 > $O/b$lz.json 2> $O/b$lz.err || { tail -20 $O/b$lz.err; exit 1; }
  echo "lazy=$lz"; grep "odom timing" $O/b$lz.err | tail -2
done

# A/B of alternative in-tree builds of libddlo_gicp.so (DDLO_GICP_LIB) on the headline leg (cfg3) and,
# with AB_CFG2=1, the cfg2 leg; each variant twice, interleaved.  Usage: bash tools/gpu_ab.sh base ab16 ab32
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${DDLO_OUT:-bench_out}/ab   # where the result lines go
mkdir -p $O
L=$PWD/dynamic_direct_lidar_odometry_amd/_lib
for rep in 1 2; do
  for v in "$@"; do
    lib=$L/libddlo_gicp.so; [ $v != base ] && lib=$L/$v/libddlo_gicp.so
    DDLO_GICP_LIB=$lib timeout -k 10 240 python -u bench.py $([ "$AB_CFG2" = 1 ] && echo --full --no-cpu --no-sharded --no-batch --no-odom --no-seg --no-walk) --steps 100 > $O/$v.json 2> $O/$v.err || { echo "FAIL $v"; tail $O/$v.err; exit 1; }
    python3 -c "import json,sys; d=json.load(open('$O/$v.json')); g=d.get('s2s_gn') or {}; print('$v', d['ms_per_step'], g.get('ms_per_align'))"
  done
done

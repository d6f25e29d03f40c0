# find_matches locality: the sort key's stream-group bits (MIB_GROUP_BITS) on one bench leg
# usage (GPU box): WL=c4 GBS="6 8 10" bash scripts/ab_group_bits.sh TAG
set -o pipefail
cd $GRAFT_REPO_ROOT
TAG=$1
O=${BENCH_OUT:-bench_out}/$TAG
mkdir -p $O
for gb in ${GBS:-6 8 10}; do
  MIB_GROUP_BITS=$gb timeout -k 10 300 python3 bench.py --workload ${WL:-c4} --full --no-cpu-baseline > $O/${WL:-c4}_g$gb.json 2> $O/${WL:-c4}_g$gb.err || { echo "g$gb failed"; tail $O/${WL:-c4}_g$gb.err; exit 1; }
  python3 -c "
import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); k=d['kernel_ms_per_step']
print(sys.argv[2], d['value'], d.get('compressed_ratio'), 'fm', k.get('find_matches'), 'sort', k.get('radix_sort'), 'dp', k.get('dp_parse'))" $O/${WL:-c4}_g$gb.json g$gb
done
echo "exit=0"

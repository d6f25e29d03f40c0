# A/B of library builds on one bench leg: bench.py with BROTLI_AMD_LIB=<each .so given>
set -o pipefail
cd $GRAFT_REPO_ROOT
TAG=$1; W=$2; shift 2
O=${BENCH_OUT:-bench_out}/$TAG
mkdir -p $O
for lib in "$@"; do
  n=$(basename $lib .so)
  BROTLI_AMD_LIB=$PWD/$lib timeout -k 10 300 python3 bench.py --workload $W --full --no-cpu-baseline > $O/${W}_$n.json 2> $O/${W}_$n.err || { echo "$n failed"; tail $O/${W}_$n.err; exit 1; }
done
echo "exit=0"

# DP variants on C4: the working build against the HEAD build (same box, same call)
set -o pipefail
cd $GRAFT_REPO_ROOT
O=${BENCH_OUT:-bench_out}/abdp
mkdir -p $O
B="timeout -k 10 400 python3 bench.py --workload c4 --full --no-cpu-baseline"
BROTLI_AMD_LIB=$PWD/brotli-lib_amd/libbrotli_amd_head.so $B > $O/head.json 2> $O/head.err || exit 1
$B > $O/work.json 2> $O/work.err || exit 1
BROTLI_AMD_LIB=$PWD/brotli-lib_amd/libbrotli_amd_head.so $B > $O/head2.json 2> $O/head2.err || exit 1
$B > $O/work2.json 2> $O/work2.err || exit 1
echo "exit=0"

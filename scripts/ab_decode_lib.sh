set -o pipefail
cd $GRAFT_REPO_ROOT
O=${BENCH_OUT:-bench_out}/abd
mkdir -p $O
timeout -k 10 600 python3 -u -m pytest tests/test_gpu_decode.py tests/test_gpu_parts.py tests/test_gpu_configs.py -m gpu -x -q --timeout 300 --timeout-method thread > $O/tests.log 2>&1 || { echo tests failed; tail -30 $O/tests.log; exit 1; }
for lib in libbrotli_amd_head libbrotli_amd; do BROTLI_AMD_LIB=$PWD/brotli-lib_amd/$lib.so timeout -k 10 400 python3 bench.py --workload c4 --full --no-cpu-baseline > $O/c4_$lib.json 2> $O/c4_$lib.err || exit 1; done
for lib in libbrotli_amd_head libbrotli_amd; do BROTLI_AMD_LIB=$PWD/brotli-lib_amd/$lib.so timeout -k 10 400 python3 bench.py --workload c3 --full --no-cpu-baseline > $O/c3_$lib.json 2> $O/c3_$lib.err || exit 1; done
echo "exit=0"

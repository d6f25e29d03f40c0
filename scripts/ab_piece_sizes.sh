# C4 / C3 / C2 bench legs at parse-piece shifts given in PS (default "3 4")
set -o pipefail
cd $GRAFT_REPO_ROOT
O=${BENCH_OUT:-bench_out}/abs
mkdir -p $O
for w in ${WL:-c4 c3 c2}; do for p in ${PS:-3 4}; do MIB_DP_PIECES=$p timeout -k 10 400 python3 bench.py --workload $w --full --no-cpu-baseline > $O/${w}_p$p.json 2> $O/${w}_p$p.err || exit 1; done; done
echo "exit=0"

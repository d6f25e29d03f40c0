# C3 (fonts) and C4 with each literal context mode forced (MIB_CTX_MODE 0 LSB6, 1 MSB6, 2 UTF8, 3 SIGNED)
set -o pipefail
cd $GRAFT_REPO_ROOT
O=${BENCH_OUT:-bench_out}/abcm
mkdir -p $O
for w in ${WL:-c3}; do for m in ${MODES:-def 0 1 2 3}; do
  if [ $m = def ]; then E=X=1; else E=MIB_CTX_MODE=$m; fi
  env $E timeout -k 10 400 python3 bench.py --workload $w --full --no-cpu-baseline > $O/${w}_$m.json 2> $O/${w}_$m.err || exit 1
done; done
echo "exit=0"

# literal prefix codes per metablock (MIB_LIT_TREES caps them) against compressed size and
# decode speed: past the decoder's LDS table area a metablock's tables stay in HBM
set -o pipefail
cd $GRAFT_REPO_ROOT
O=${BENCH_OUT:-bench_out}/ablt
mkdir -p $O
for w in ${WL:-c3 c4}; do for c in ${CAPS:-64 32 24}; do
  MIB_LIT_TREES=$c timeout -k 10 400 python3 bench.py --workload $w --full --no-cpu-baseline > $O/${w}_$c.json 2> $O/${w}_$c.err || exit 1
done; done
echo "exit=0"

# FETCH_SIZE / WRITE_SIZE of `RTGPU_LANES=1 python bench.py` (separate runs, kernel-trace only)
cd $GRAFT_REPO_ROOT
RUNS=${RUNS:-runs}   # where the run records go
export TMPDIR=/tmp
T=${1:-v19}
mkdir -p $RUNS/$T
for c in FETCH_SIZE WRITE_SIZE; do
  RTGPU_LANES=1 timeout 600 rocprofv3 --kernel-trace --pmc $c -d $RUNS/$T/p_$c -o r -- python bench.py --full --no-cpu-baseline > /dev/null 2>&1
  python tools/rocpd_summary.py $(find $RUNS/$T/p_$c -name '*.db' | head -1) > $RUNS/$T/pmc_$c.txt
  grep -i "k_trace\|k_shade" $RUNS/$T/pmc_$c.txt | tail -3
  rm -rf $RUNS/$T/p_$c
done

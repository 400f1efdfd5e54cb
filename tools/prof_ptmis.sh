# PathTracerMIS evidence set: default bench, serial kernel stats, FETCH_SIZE / WRITE_SIZE passes (separate runs, kernel-trace only)
set -x
cd $GRAFT_REPO_ROOT
RUNS=${RUNS:-runs}   # where the run records go
export TMPDIR=/tmp
T=${1:-v15}
mkdir -p $RUNS/$T
python bench.py --full > $RUNS/$T/bench_default.json 2>/dev/null
tail -1 $RUNS/$T/bench_default.json | cut -c1-400
RTGPU_LANES=1 rocprofv3 --kernel-trace --stats -d $RUNS/$T/p1 -o r -- python bench.py --full --no-cpu-baseline > $RUNS/$T/bench_serial_profiled.json 2>/dev/null
python tools/rocpd_summary.py $(find $RUNS/$T/p1 -name '*.db' | head -1) > $RUNS/$T/kernel_stats_serial.txt
head -8 $RUNS/$T/kernel_stats_serial.txt
for c in FETCH_SIZE WRITE_SIZE; do
  RTGPU_LANES=1 rocprofv3 --kernel-trace --pmc $c -d $RUNS/$T/p_$c -o r -- python bench.py --full --no-cpu-baseline > /dev/null 2>&1
  python tools/rocpd_summary.py $(find $RUNS/$T/p_$c -name '*.db' | head -1) > $RUNS/$T/pmc_$c.txt
  grep -i "k_trace\|k_shade" $RUNS/$T/pmc_$c.txt | tail -6
done
rm -rf $RUNS/$T/p1 $RUNS/$T/p_FETCH_SIZE $RUNS/$T/p_WRITE_SIZE

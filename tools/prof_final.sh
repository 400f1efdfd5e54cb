# end-of-round evidence: default bench, the same command under rocprofv3 (serial lanes), GPU tests, VCM throughput + kernel stats
set -x
cd $GRAFT_REPO_ROOT
RUNS=${RUNS:-runs}   # where the run records go
export TMPDIR=/tmp
T=${1:-v18}
mkdir -p $RUNS/$T
python bench.py --full > $RUNS/$T/bench_default.json 2> $RUNS/$T/bench_default.err
tail -1 $RUNS/$T/bench_default.json | cut -c1-400
RTGPU_LANES=1 rocprofv3 --kernel-trace --stats -d $RUNS/$T/prof_serial -o r -- python bench.py --full --no-cpu-baseline > $RUNS/$T/bench_serial_profiled.json 2>/dev/null
python tools/rocpd_summary.py $(find $RUNS/$T/prof_serial -name '*.db' | head -1) > $RUNS/$T/kernel_stats_serial.txt
head -8 $RUNS/$T/kernel_stats_serial.txt
python -c "
import json
d=json.loads(open('$RUNS/$T/bench_serial_profiled.json').read().strip().splitlines()[-1])
print('HIP events avg_launch_ms', d['roofline']['avg_launch_ms'], 'launches', d['roofline']['launches'])"
python -m pytest tests -q -m gpu 2>&1 | tail -3 > $RUNS/$T/pytest_gpu.log; cat $RUNS/$T/pytest_gpu.log
python tools/bench_vcm.py --passes 16 > $RUNS/$T/vcm_caustics.json 2>/dev/null; tail -1 $RUNS/$T/vcm_caustics.json | cut -c1-300
python tools/bench_vcm.py --passes 16 --no-merging > $RUNS/$T/vcm_caustics_bdpt.json 2>/dev/null; tail -1 $RUNS/$T/vcm_caustics_bdpt.json | cut -c1-300
python tools/bench_vcm.py --scene sponza --passes 16 > $RUNS/$T/vcm_sponza.json 2>/dev/null; tail -1 $RUNS/$T/vcm_sponza.json | cut -c1-300
python tools/bench_vcm.py --scene sponza --passes 16 --no-merging > $RUNS/$T/vcm_sponza_bdpt.json 2>/dev/null; tail -1 $RUNS/$T/vcm_sponza_bdpt.json | cut -c1-300
rocprofv3 --kernel-trace --stats -d $RUNS/$T/prof_vcm -o r -- python tools/bench_vcm.py --passes 16 > /dev/null 2>&1
python tools/rocpd_summary.py $(find $RUNS/$T/prof_vcm -name '*.db' | head -1) > $RUNS/$T/vcm_kernel_stats_caustics.txt
head -9 $RUNS/$T/vcm_kernel_stats_caustics.txt
rm -rf $RUNS/$T/prof_serial $RUNS/$T/prof_vcm

set -x
cd $GRAFT_REPO_ROOT
RUNS=${RUNS:-runs}   # where the run records go
export TMPDIR=/tmp
mkdir -p $RUNS/v13
python bench.py --full > $RUNS/v13/bench_default.json 2> $RUNS/v13/bench_default.err
tail -1 $RUNS/v13/bench_default.json | cut -c1-600
RTGPU_LANES=1 rocprofv3 --kernel-trace --stats -d $RUNS/v13/prof_serial -o r -- python bench.py --full > $RUNS/v13/bench_serial_profiled.json 2>/dev/null
python tools/rocpd_summary.py $(find $RUNS/v13/prof_serial -name '*.db' | head -1) > $RUNS/v13/kernel_stats_serial.txt
head -12 $RUNS/v13/kernel_stats_serial.txt
python tools/bench_vcm.py > $RUNS/v13/vcm_caustics.json 2>/dev/null; tail -1 $RUNS/v13/vcm_caustics.json
python tools/bench_vcm.py --scene sponza --passes 16 > $RUNS/v13/vcm_sponza.json 2>/dev/null; tail -1 $RUNS/v13/vcm_sponza.json
python tools/bench_vcm.py --scene sponza --passes 16 --no-merging > $RUNS/v13/vcm_sponza_bdpt.json 2>/dev/null; tail -1 $RUNS/v13/vcm_sponza_bdpt.json
rocprofv3 --kernel-trace --stats -d $RUNS/v13/prof_vcm -o r -- python tools/bench_vcm.py --scene sponza > /dev/null 2>&1
python tools/rocpd_summary.py $(find $RUNS/v13/prof_vcm -name '*.db' | head -1) > $RUNS/v13/vcm_kernel_stats_sponza.txt
head -24 $RUNS/v13/vcm_kernel_stats_sponza.txt
rocprofv3 --kernel-trace --stats -d $RUNS/v13/prof_vcm2 -o r -- python tools/bench_vcm.py > /dev/null 2>&1
python tools/rocpd_summary.py $(find $RUNS/v13/prof_vcm2 -name '*.db' | head -1) > $RUNS/v13/vcm_kernel_stats_caustics.txt
head -24 $RUNS/v13/vcm_kernel_stats_caustics.txt
python -m pytest tests -q -m gpu 2>&1 | tail -3 > $RUNS/v13/pytest_gpu.log; cat $RUNS/v13/pytest_gpu.log
rm -rf $RUNS/v13/prof_serial $RUNS/v13/prof_vcm $RUNS/v13/prof_vcm2

set -x
R=$PWD
mkdir -p "${1:?usage: bash tools/refresh_profiles.sh OUT_DIR}"; OUT=$(cd "$1" && pwd)  # absolute: the script changes directory
python bench.py --full > $OUT/bench.json 2> $OUT/bench.err
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d /tmp/p1 -o p1 -- python $R/bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-kernel-timing > $OUT/bench_under_rocprof.json 2>/dev/null
python $R/tools/rocprof_summary.py $(find /tmp/p1 -name "*.db" | head -1) > $OUT/kernel_trace_summary.txt 2>&1
TRAIN_GRAPH=0 rocprofv3 --kernel-trace --stats -d /tmp/p2 -o p2 -- python $R/tools/train_step_time.py > $OUT/train_step.txt 2>/dev/null
python $R/tools/rocprof_summary.py $(find /tmp/p2 -name "*.db" | head -1) > $OUT/train_kernel_trace_summary.txt 2>&1
cd $R; python tools/train_step_time.py > $OUT/train_step_plain.txt 2>&1
tail -2 $OUT/train_step_plain.txt
head -c 600 $OUT/bench.json

# kernel trace of one non-pipelined config-2 step, per-batch breakdown
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
O=${OUT_DIR:-bench_out}/tr
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats -T -f csv -d $O -o run -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-pipeline > $O/bench.json 2> $O/bench.err
python3 tools/trace_batches.py $O/run_kernel_trace.csv

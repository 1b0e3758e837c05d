set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
O=${OUT_DIR:-bench_out}/trp
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace -f csv -d $O -o run -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > $O/bench.json 2> $O/bench.err || exit 1
python3 tools/trace_overlap.py $O/run_kernel_trace.csv

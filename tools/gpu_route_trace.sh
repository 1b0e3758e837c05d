# kernel trace of the routed config-2 path on one rank (bench --route): where
# the step goes beyond the engine's own kernels (pack, RCCL, unpack, host gaps)
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
O=${OUT_DIR:-bench_out}/rtr
mkdir -p $O
timeout -k 10 400 rocprofv3 --kernel-trace --stats -f csv -d $O -o run -- python3 bench.py --full --route --steps 2 --warmup 1 --no-cpu-baseline > $O/bench.json 2> $O/bench.err || exit 1
f=$(find $O -name 'run_kernel_trace.csv' | head -1)
python3 tools/trace_busy.py "$f" --from-kernel k_init_segments > $O/busy.txt && cat $O/busy.txt

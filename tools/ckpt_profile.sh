# usage: bash tools/ckpt_profile.sh <output dir> -- the default bench line with its extras (--full), then rocprofv3 passes
# of the plain command, each pass its own run
set -e
OUT=$(realpath -m "${1:?usage: tools/ckpt_profile.sh <output dir>}")
mkdir -p "$OUT/prof"
export TMPDIR=${TMPDIR:-/tmp}
cd "$(dirname "$0")/.."
timeout -k 10 600 python bench.py --full > "$OUT/bench_default.log" 2> "$OUT/bench_default.err"
echo bench done > "$OUT/progress.txt"
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof/stats" -o run -- python3 bench.py > "$OUT/bench_under_rocprof.log" 2> "$OUT/rocprof_stats.err"
echo stats done >> "$OUT/progress.txt"
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE -d "$OUT/prof/pmc_fetch" -o run -- python3 bench.py --reads-per-gap 100 > "$OUT/bench_pmc_fetch.log" 2> "$OUT/rocprof_pmc1.err"
echo pmc1 done >> "$OUT/progress.txt"
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE -d "$OUT/prof/pmc_write" -o run -- python3 bench.py --reads-per-gap 100 > "$OUT/bench_pmc_write.log" 2> "$OUT/rocprof_pmc2.err"
echo pmc2 done >> "$OUT/progress.txt"
timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE -d "$OUT/prof/pmc_fetch_def" -o run -- python3 bench.py > "$OUT/bench_pmc_fetch_def.log" 2> "$OUT/rocprof_pmc3.err"
echo pmc3 done >> "$OUT/progress.txt"
timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE -d "$OUT/prof/pmc_write_def" -o run -- python3 bench.py > "$OUT/bench_pmc_write_def.log" 2> "$OUT/rocprof_pmc4.err"
echo pmc4 done >> "$OUT/progress.txt"
ls -R "$OUT/prof" | head -30

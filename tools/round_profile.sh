# Round-end evidence for the default bench line with every sub-record (--full): the bench JSON,
# the rocprofv3 kernel-trace summary of the SAME command, the PMC traffic passes (FETCH_SIZE /
# WRITE_SIZE, tools/pmc_traffic.sh, which keeps its own folder) and the effective-clock pass
# (GRBM_GUI_ACTIVE).  Usage: bash tools/round_profile.sh <tag>; files go to $OUT (bench_out).
set -u
tag=${1:-latest}
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 400 python bench.py --full > "$OUT/bench_$tag.json" 2> "$OUT/bench_$tag.err" || exit $?
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$tag" -o run --output-format csv -- python3 bench.py --full > "$OUT/prof_$tag.log" 2>&1 || exit $?
bash tools/pmc_traffic.sh || exit $?
timeout -s KILL 300 rocprofv3 --pmc GRBM_GUI_ACTIVE GRBM_COUNT --output-format csv -d "$OUT/pmc_clk" -o c -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-ttk > "$OUT/pmc_clk.log" 2>&1 || exit $?
echo done

# Bench lines (--full: stage split, time-to-k, sub-records) for every workload the repo claims
# numbers for (C4a fp64 / fp32 basis, C4b R-MAT, C2, host spill); each to $OUT/ev_<name>.json
# (OUT defaults to bench_out).  Usage: bash tools/evidence.sh
set -u
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
run() {
  name=$1; shift
  timeout -k 10 600 python bench.py --full "$@" > "$OUT/ev_$name.json" 2> "$OUT/ev_$name.err" || exit $?
  echo "$name: $(python3 -c "import json,sys;d=json.load(open(sys.argv[1]));print(d['value'], d['unit'])" "$OUT/ev_$name.json")"
}
run c4a_fp64 --steps 3 --no-cpu-baseline
run c4a_fp32 --basis-bits 32 --steps 3 --no-cpu-baseline
run c4b_rmat --matrix rmat --steps 2 --no-cpu-baseline
run c2_b16 --n 1000000 --b 16 --halfwidth 32 --steps 5 --no-cpu-baseline
run c4a_spill20 --device-blocks 20 --steps 1 --no-cpu-baseline --no-ttk

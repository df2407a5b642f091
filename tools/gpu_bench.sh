# The bench with every sub-record (--full) at C2's shape, then at the default C4a.  Logs go to
# $OUT (default bench_out/).
set -u
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 300 python bench.py --full --n 1000000 --b 16 --k 20 --steps 2 --no-cpu-baseline > "$OUT/b1.log" 2>&1; rc=$?
echo "bench small rc=$rc"
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 900 python bench.py --full --steps 2 > "$OUT/b2.log" 2>&1; rc=$?
echo "bench full rc=$rc"
exit $rc

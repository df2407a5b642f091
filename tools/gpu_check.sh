# GPU round check: parity tests, then the bench (--full: every sub-record), then a rocprofv3
# kernel trace of the bench.  Logs go to $OUT (default bench_out/).
set -u
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -q -x --timeout 300 --timeout-method thread > "$OUT/t1.log" 2>&1; rc=$?
echo "pytest rc=$rc"; tail -3 "$OUT/t1.log"
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 900 python bench.py --full --steps 2 > "$OUT/b2.log" 2>&1; rc=$?
echo "bench rc=$rc"; tail -c 3000 "$OUT/b2.log"
if [ $rc -ne 0 ]; then exit $rc; fi
if [ "${PROFILE:-1}" = "1" ]; then
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-ttk > "$OUT/prof.log" 2>&1; rc=$?
echo "rocprof rc=$rc"
fi
exit $rc

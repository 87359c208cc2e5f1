set -u
cd "$(dirname "$0")/.."
OUT="${OUT:-build/gpu_check}"
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread >"$OUT/pytest_gpu.log" 2>&1
rc=$?
echo "pytest rc=$rc"
tail -5 "$OUT/pytest_gpu.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python -u bench.py --full --steps 20 --warmup 5 --cpu-seconds 8 > "$OUT/bench.log" 2>&1
rc2=$?
echo "bench rc=$rc2"
tail -3 "$OUT/bench.log"
exit $rc2

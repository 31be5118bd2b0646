# The driver's bench command and the default one, every row and leg (--full), logs under $OUT
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 400 python -u bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_driver.log 2>&1; rc=$?
echo "driver-style bench rc=$rc"; grep "^\[bench\]" $OUT/bench_driver.log; [ $rc -ne 0 ] && { tail -20 $OUT/bench_driver.log; exit $rc; }
timeout -k 10 500 python -u bench.py --full ${ARGS:-} > $OUT/bench_default.log 2>&1; rc=$?
echo "default bench rc=$rc"; grep "^\[bench\]" $OUT/bench_default.log
exit $rc

# The GPU suite, the smoke check and the default bench line (bench.py --full: with the kernel
# table, the roofline, the C4 leg and the CPU baseline) on this tree; logs go to $LOGS (./logs).
# pytest exit 1 (test failures) continues to the smoke and the bench; any other non-zero status
# (a crash, an abort, a time limit) ends the script.
set -e
set -o pipefail
LOGS=${LOGS:-logs}
mkdir -p $LOGS
export AEROGNN_MEMLOG=0
T=${1:-r4a}
rc=0
timeout -k 10 900 python -u -m pytest tests -m gpu -v -rP --timeout 300 --timeout-method thread \
    > $LOGS/${T}_gpu_tests.log 2>&1 || rc=$?
tail -3 $LOGS/${T}_gpu_tests.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "gpu tests ended with status $rc"; exit $rc; fi
grep -q "Memory access fault\|Fatal Python error\|core dumped" $LOGS/${T}_gpu_tests.log && exit 3
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $LOGS/${T}_smoke.log 2>&1
tail -2 $LOGS/${T}_smoke.log
timeout -k 10 600 python -u bench.py --full --steps 20 --warmup 5 > $LOGS/${T}_bench.log 2>&1
tail -1 $LOGS/${T}_bench.log | cut -c1-400

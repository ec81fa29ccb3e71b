#!/bin/bash
# One GPU-box visit: smoke, GPU parity tests, bench, rocprofv3 kernel stats.  Outputs -> $TOOLS_OUT (default tools_out/).
set -u
cd "$(dirname "$0")/.."
TOOLS_OUT="${TOOLS_OUT:-tools_out}"; export TOOLS_OUT; mkdir -p "$TOOLS_OUT"
export TMPDIR=/tmp
{ nproc; lscpu | grep -E "Model name|Socket|Core|Thread"; rocm-smi --showproductname 2>/dev/null | head -8; } > $TOOLS_OUT/env.log 2>&1
echo "== smoke"; timeout 600 python -c "import __graft_entry__ as g; g.smoke()" > $TOOLS_OUT/smoke.log 2>&1; echo "smoke rc=$?"; tail -3 $TOOLS_OUT/smoke.log
echo "== pytest -m gpu"; timeout 1500 python -m pytest tests -m gpu -q --timeout 600 > $TOOLS_OUT/pytest_gpu.log 2>&1; echo "pytest rc=$?"; tail -15 $TOOLS_OUT/pytest_gpu.log
echo "== bench"; timeout 600 python bench.py --full --steps 10 --warmup 3 > $TOOLS_OUT/bench.log 2> $TOOLS_OUT/bench.err; echo "bench rc=$?"; cat $TOOLS_OUT/bench.log; tail -5 $TOOLS_OUT/bench.err
if [ "${1:-}" != "noprof" ]; then
  echo "== rocprofv3"; ( cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OLDPWD/$TOOLS_OUT/prof" -o r02 -- python "$OLDPWD/bench.py" --steps 40 --warmup 10 --no-cpu-baseline --no-prof --no-stream-inputs --secondary none --secondary none > "$OLDPWD/$TOOLS_OUT/rocprof.log" 2>&1 ); echo "rocprof rc=$?"
  find $TOOLS_OUT/prof -name "*kernel_stats*" | head; f=$(find $TOOLS_OUT/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -25 "$f"
  # keep only the small summaries (the traces are large)
  find $TOOLS_OUT/prof -name "*kernel_trace.csv" -size +20M -delete
fi

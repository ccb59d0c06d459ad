#!/bin/bash
# Round 6 (late): a multi-problem F(4x4) launch's blocks ordered by falling Cin (SA_W4_ORDER=1, the
# built library) against the caller's order (variants/w4noorder.so, -DSA_W4_ORDER=0): the wino4 /
# model parity tests, then forward lines interleaved three times
cd "$GRAFT_REPO_ROOT" || exit 2
OUT=${OUT:-ab_out/w4o}   # where the logs and the summary go
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest -x -q --timeout 120 --timeout-method thread tests/test_gpu_wino.py tests/test_gpu_model.py > $OUT/tests.log 2>&1 || exit 1
for pass in 1 2 3; do
  for v in order caller; do
    if [ $v = caller ]; then export SA_HIP_LIB=variants/w4noorder.so; else unset SA_HIP_LIB; fi
    timeout -k 10 300 python bench.py --full --steps 8 --warmup 3 --no-cpu-baseline --no-epe > $OUT/f_${v}_$pass.log 2>&1 || exit 1
    tail -n 1 $OUT/f_${v}_$pass.log | python -c '
import sys, json
d = json.loads(sys.stdin.read()); k = d["roofline"]["kernels"]
print(sys.argv[1], round(d["value"], 2), round(d["ms_per_step"], 2), "w4", round(k["conv2d_wino4"]["ms_per_step"], 2), "one-stream", round(d["roofline"]["one_stream_ms_per_step"], 2))' "$v" >> $OUT/summary.txt
  done
done

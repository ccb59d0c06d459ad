#!/bin/bash
# Round 6 (late): every source compiled with the wave-priority pass (variants/allprio.so from
# scripts/build_all_variant.sh allprio -mllvm -amdgpu-set-wave-priority) against the built library
# (the pass on conv2d_wino4 only): the whole GPU suite on the variant, then forward lines interleaved three times
cd "$GRAFT_REPO_ROOT" || exit 2
OUT=${OUT:-ab_out/allp}   # where the logs and the summary go
mkdir -p "$OUT"
V=${1:-variants/allprio.so}
SA_HIP_LIB=$V timeout -k 10 400 python -u -m pytest -x -q --timeout 120 --timeout-method thread tests -m gpu > $OUT/tests.log 2>&1 || exit 1
for pass in 1 2 3; do
  for v in built variant; do
    if [ $v = variant ]; then export SA_HIP_LIB=$V; else unset SA_HIP_LIB; fi
    timeout -k 10 300 python bench.py --full --steps 8 --warmup 3 --no-cpu-baseline --no-epe > $OUT/f_${v}_$pass.log 2>&1 || exit 1
    tail -n 1 $OUT/f_${v}_$pass.log | python -c '
import sys, json
d = json.loads(sys.stdin.read()); k = d["roofline"]["kernels"]
print(sys.argv[1], round(d["value"], 2), round(d["ms_per_step"], 2), "w4", round(k["conv2d_wino4"]["ms_per_step"], 2), "one-stream", round(d["roofline"]["one_stream_ms_per_step"], 2))' "$v" >> $OUT/summary.txt
  done
done

#!/bin/bash
# Full measurement pass on the GPU box (outputs under $OUT, an absolute path; default prof_out/):
#   bench      the bench line with --full (value, roofline, cpu baseline)
#   trace      rocprofv3 --kernel-trace --stats over a short bench run (hipGraph replays)
#   trace1s    the same with every step eager on one stream, the whole batch per launch
#              (bench.py --one-stream: the instrumented steps' schedule, per-launch times comparable)
#   fetch/write  rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate runs (HBM bytes, --one-stream)
#   trace5     the one-stream kernel trace of a cfg5 step (the booster batch)
#   cfg3/4/5   the other configs' bench lines
#   dist2      a 2-rank torchrun rehearsal of the bench on one GPU (gloo, ranks share the card)
# Each step under its own limit; a fault or time-out ends the script (gpu_steps.sh).
# usage: scripts/profile_round.sh [a|b|all]
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 2
R=$(pwd)
OUT=${OUT:-$R/prof_out}   # where the logs, lines and traces go
mkdir -p "$OUT"
SHORT="python3 $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-epe"
exec_steps=(
  "bench:420:python3 $R/bench.py --full > $OUT/bench.log 2>&1; tail -n 1 $OUT/bench.log > $OUT/bench.json"
  "trace:300:cd /tmp && rocprofv3 --kernel-trace --stats -d $OUT/trace -o run --output-format csv -- $SHORT"
  "trace1s:300:cd /tmp && rocprofv3 --kernel-trace --stats -d $OUT/trace1s -o run --output-format csv -- $SHORT --one-stream"
  "fetch:300:cd /tmp && rocprofv3 --pmc FETCH_SIZE -d $OUT/fetch -o run --output-format csv -- $SHORT --one-stream"
  "write:300:cd /tmp && rocprofv3 --pmc WRITE_SIZE -d $OUT/write -o run --output-format csv -- $SHORT --one-stream"
  "trace5:400:cd /tmp && rocprofv3 --kernel-trace --stats -d $OUT/trace5 -o run --output-format csv -- python3 $R/bench.py --config cfg5 --steps 1 --warmup 1 --no-cpu-baseline --no-epe --one-stream"
  "cfg3:300:python3 $R/bench.py --config cfg3 --full > $OUT/cfg3.log 2>&1; tail -n 1 $OUT/cfg3.log > $OUT/bench_cfg3.json"
  "cfg4:300:python3 $R/bench.py --config cfg4 --full > $OUT/cfg4.log 2>&1; tail -n 1 $OUT/cfg4.log > $OUT/bench_cfg4.json"
  "cfg5:420:python3 $R/bench.py --config cfg5 --full > $OUT/cfg5.log 2>&1; tail -n 1 $OUT/cfg5.log > $OUT/bench_cfg5.json"
  "dist2:300:cd $R && SA_DIST_BACKEND=gloo SA_DIST_SHARE_GPU=1 python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --config cfg4 --steps 2 --warmup 1 --full --no-epe > $OUT/dist2.log 2>&1"
)
# part a / b (one gpurun call each: a call is limited to 20 minutes): the first five steps / the rest
case "${1:-all}" in
  a) bash "$R/scripts/gpu_steps.sh" "${exec_steps[@]:0:5}" ;;
  b) bash "$R/scripts/gpu_steps.sh" "${exec_steps[@]:5}" ;;
  *) bash "$R/scripts/gpu_steps.sh" "${exec_steps[@]}" ;;
esac

#!/usr/bin/env python3
"""forward(test_mode=False) at the bench config (B = 4 pairs 544x960, 22 iterations): ms per forward
of the test-mode forward, the full-outputs forward with the fused mask head + up-sampling
(ScheduleOptions.fuse_mask_upsample, the default) and with the unfused pair, alternating; and, per
call at that shape (4 x 256 x 136 x 240), sa_mask_upsample against sa_conv1x1 + sa_convex_upsample
beside their bytes models.

    python scripts/bench_full_outputs.py [steps [rounds]]   (default 5 steps, 3 rounds)"""
import dataclasses
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from stereoanywhere_amd import ops, synth  # noqa: E402
from stereoanywhere_amd.model import StereoAnywhere  # noqa: E402

B, H, W, ITERS = 4, 544, 960, 22


def timeit(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000 / reps


def per_call(dev):
    """us per call at the bench shape's 1/4 resolution, on mask-head-like inputs."""
    H4, W4, Cin = H // 4, W // 4, 256
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.relu(torch.randn(B, Cin, H4, W4, device=dev, generator=g))
    w = 0.05 * torch.randn(144, Cin, 1, 1, device=dev, generator=g)
    bias = torch.randn(144, device=dev, generator=g)
    flow = 5 * torch.randn(B, 1, H4, W4, device=dev, generator=g)
    ws = ops.conv1x1_weights(w)
    out = torch.empty(B, 1, H, W, device=dev)
    mask = torch.empty(B, 144, H4, W4, device=dev)
    npx = B * H4 * W4
    b_x, b_mask, b_out, b_flow = 4.0 * npx * Cin, 4.0 * npx * 144, 4.0 * npx * 16, 4.0 * npx
    rows = []
    for rnd in range(3):   # alternating: the three kernels see the same box state
        t_f = timeit(lambda: ops.mask_upsample(x, ws, bias, 0.25, flow, out=out))
        t_c = timeit(lambda: ops.conv1x1(x, ws, 144, bias, 0.25, out=mask))
        t_u = timeit(lambda: ops.convex_upsample(flow, mask, 4, out=out))
        rows.append((t_f, t_c, t_u))
        print(f"  round {rnd}: mask_upsample {t_f:7.1f} us | conv1x1 {t_c:7.1f} us + convex_upsample {t_u:7.1f} us "
              f"= {t_c + t_u:7.1f} us", flush=True)
    t_f, t_c, t_u = (min(r[i] for r in rows) for i in range(3))
    m_f, m_c, m_u = b_x + b_flow + b_out, b_x + b_mask, b_mask + b_flow + b_out
    print(f"  bytes model: mask_upsample {m_f / 1e6:.0f} MB ({m_f / t_f / 1e6:.2f} TB/s at the best round) | "
          f"conv1x1 {m_c / 1e6:.0f} MB ({m_c / t_c / 1e6:.2f} TB/s) + convex_upsample {m_u / 1e6:.0f} MB "
          f"({m_u / t_u / 1e6:.2f} TB/s)", flush=True)
    ref = ops.convex_upsample(flow, ops.conv1x1(x, ws, 144, bias, 0.25), 4)
    got = ops.mask_upsample(x, ws, bias, 0.25, flow)
    print(f"  fused vs unfused on these inputs: max|d| {float((got - ref).abs().max()):.2e}, "
          f"bit-identical {torch.equal(got, ref)}", flush=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    steps = int(args[0]) if args else 5
    rounds = int(args[1]) if len(args) > 1 else 3
    dev = torch.device("cuda", 0)
    sysfs = bench._gpu_sysfs(dev)
    print("box before:", json.dumps(bench.box_state(sysfs)), json.dumps(bench.clock_probe(dev)), flush=True)
    model = StereoAnywhere(dict(bench.PUBLISHED, volume_corruption_prob=0)).eval()
    synth.load_seeded_weights(model, 0)
    model = model.to(dev)
    inp = bench.make_inputs(B, 540, 960, H, W, 192.0, seed0=1, device=dev)
    x = (inp["left"], inp["right"], inp["mono_left"], inp["mono_right"])
    base = model.opts
    modes = [("test_mode=True", True, True), ("full outputs, fused", False, True),
             ("full outputs, unfused", False, False)]
    last = {}
    with torch.no_grad():
        for name, test_mode, fuse in modes:   # one warm-up of every mode
            model.opts = dataclasses.replace(base, fuse_mask_upsample=fuse)
            model(*x, iters=ITERS, test_mode=test_mode)
        torch.cuda.synchronize()
        print(f"forward B{B} {H}x{W}, {ITERS} iterations, {steps} steps per window:", flush=True)
        for rnd in range(rounds):
            for name, test_mode, fuse in modes:
                model.opts = dataclasses.replace(base, fuse_mask_upsample=fuse)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    out = model(*x, iters=ITERS, test_mode=test_mode)[0]
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / steps * 1e3
                last[name] = out if test_mode else out[-1]
                print(f"  round {rnd} {name:22s} {dt:8.2f} ms/forward", flush=True)
    ref = last["test_mode=True"]
    for name in ("full outputs, fused", "full outputs, unfused"):
        print(f"  last prediction of '{name}' vs test mode: max|d| {float((last[name] - ref).abs().max()):.2e}",
              flush=True)
    model.opts = base
    print(f"per call, {B}x256x{H // 4}x{W // 4} -> {B}x1x{H}x{W}:", flush=True)
    per_call(dev)
    print("box after:", json.dumps(bench.box_state(sysfs)), json.dumps(bench.clock_probe(dev)), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The hourglass's stride-1 3x3x3 convs (stereoanywhere_amd.diffops.conv3d_k3: csrc/conv3d_mfma.hip forward and
data gradient, csrc/conv3d_backward.hip weight gradient) beside torch's F.conv3d on the same GPU, at the bench
shape's three volumes: 4 x 8 x 240 x 136 x 240, 4 x 16 x 120 x 68 x 120 and 4 x 32 x 60 x 34 x 60.  Forward (no
grad), the data gradient's and the weight gradient's launches alone (each with its own scale launch) and
forward + backward through autograd: time per call (10 calls between two events after a warm-up), the ratio to
torch, TF/s of 2 x 27 x C x C x cells flops per direction and TB/s of the bytes model.  Inputs rotate over
several volumes so that each call's arrive from HBM, not from the 256 MiB Infinity Cache.  torch's dx and dw
alone are torch.autograd.grad with respect to one leaf, less the forward.

Bytes model, in volumes (x, g, out, dx all one volume V): forward x + out = 2 V; dx g (scale) + g + dx = 3 V;
dw g (scale) + x + g = 3 V; forward + backward 8 V less the shared scale launch's V = 7 V.

    python scripts/bench_conv3d_backward.py            the timing table
    python scripts/bench_conv3d_backward.py --memory   held and peak memory of one forward + backward of
                                                       blocks.Hourglass at 1 x 8 x 240 x 136 x 240 with closes="hip",
                                                       joins="hip", without and with convs="hip" """
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from stereoanywhere_amd import blocks, diffops, ops  # noqa: E402

# (B, C, (D, H, W))
CASES = ((4, 8, (240, 136, 240)), (4, 16, (120, 68, 120)), (4, 32, (60, 34, 60)))


def measure(fn, reps=10):
    fn()
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3   # microseconds


def torch_conv(x, weight, x_bounded=True):
    return F.conv3d(x, weight, padding=1)


def timings():
    d = torch.device("cuda", 0)
    print("3x3x3 conv, Cin = Cout: HIP / torch F.conv3d in microseconds per call", flush=True)
    print(f"  {'case':<36s} {'HIP us':>10s} {'torch us':>10s} {'ratio':>7s} {'HIP TF/s':>9s} {'MB model':>9s} {'HIP TB/s':>9s}")
    for B, C, size in CASES:
        gen = torch.Generator(device=d).manual_seed(0)
        n = size[0] * size[1] * size[2]
        v_mb, gf = B * C * n * 4 / 1e6, 2.0 * 27 * C * C * B * n / 1e9
        ROT = max(2, int(640 / (2 * v_mb)) + 1)
        sets = [(torch.randn((B, C) + size, device=d, generator=gen), torch.randn((B, C) + size, device=d, generator=gen))
                for _ in range(ROT)]
        weight = torch.randn((C, C, 3, 3, 3), device=d, generator=gen) * (2.0 / (27 * C)) ** 0.5
        w_dx = weight.reshape(C, C, 27).flip(2).permute(0, 2, 1).contiguous()
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % ROT
            return sets[turn[0]]

        def line(what, hip_us, torch_us, flops_gf, mb):
            print(f"  {what:<36s} {hip_us:10.1f} {torch_us:10.1f} {torch_us / hip_us:7.2f} {flops_gf / hip_us * 1e3:9.2f} "
                  f"{mb:9.1f} {mb / hip_us:9.2f}", flush=True)

        def hip_dx():
            g = nxt()[1]
            return ops.conv3d_mf_scaled(g, ops.conv3d_mf_table(w_dx), *ops.sample_scale(g, C))

        def hip_dw():
            x, g = nxt()
            return ops.conv3d_k3_backward_weight(x, g, None, ops.sample_scale(g, 1)[0])

        def fb(conv, leaves_of):
            x, g = nxt()
            leaves = leaves_of(x)
            out = conv(x, weight, x_bounded=True)
            grads = torch.autograd.grad(out, leaves, g) if g is not None else None
            for t in leaves:
                t.requires_grad_(False)
            return grads

        def grad_fwd(leaves_of):
            x, _ = nxt()
            leaves = leaves_of(x)
            out = torch_conv(x, weight)
            for t in leaves:
                t.requires_grad_(False)
            return out

        both = lambda x: [x.requires_grad_(True), weight.requires_grad_(True)]   # noqa: E731
        only_x = lambda x: [x.requires_grad_(True)]                              # noqa: E731
        only_w = lambda x: [weight.requires_grad_(True)]                         # noqa: E731

        print(f" conv {B} x {C} -> {C} x {'x'.join(map(str, size))} (a volume {v_mb:.0f} MB, {gf:.0f} GF per direction; "
              f"{ROT} in rotation)", flush=True)
        with torch.no_grad():
            hip_f = measure(lambda: diffops.conv3d_k3(nxt()[0], weight, x_bounded=True))
            ref_f = measure(lambda: torch_conv(nxt()[0], weight))
        line("forward", hip_f, ref_f, gf, 2 * v_mb)
        line("dx (launches alone)", measure(hip_dx), measure(lambda: fb(torch_conv, only_x)) - measure(lambda: grad_fwd(only_x)),
             gf, 3 * v_mb)
        line("dw (launches alone)", measure(hip_dw), measure(lambda: fb(torch_conv, only_w)) - measure(lambda: grad_fwd(only_w)),
             gf, 3 * v_mb)
        line("forward + backward (autograd)", measure(lambda: fb(diffops.conv3d_k3, both)),
             measure(lambda: fb(torch_conv, both)), 3 * gf, 7 * v_mb)
        del sets


def memory():
    d = torch.device("cuda", 0)
    torch.manual_seed(0)
    D, H, W = 240, 136, 240
    fc = (1, 1, 128, 128, 128, 128)
    hg = blocks.Hourglass(8, 8, feature_channels=fc).to(d)
    x = torch.randn(1, 8, D, H, W, device=d)
    fl = [torch.randn(1, fc[2 + i], H >> i, W >> i, device=d) for i in range(3)]
    fr = [torch.randn(1, fc[2 + i], H >> i, D >> i, device=d) for i in range(3)]
    g = torch.randn(1, 8, D, H, W, device=d)
    vol_mb = x.numel() * 4 / 1e6
    print(f"one forward + backward of the hourglass at 1x8x{D}x{H}x{W} (a full-resolution volume {vol_mb:.0f} MB)",
          flush=True)
    for name, convs in (("closes='hip', joins='hip'", None), ("... and convs='hip'", "hip")):
        for step in range(2):   # the second step is the one reported: the first also holds MIOpen's workspaces' search
            hg.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = hg(x, fl, fr, closes="hip", joins="hip", convs=convs)
            held = torch.cuda.memory_allocated() - base
            (out * g).sum().backward()
            b.record()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            del out
        print(f"  {name:<28s} held after the forward {held / 1e6:9.0f} MB = {held / 1e6 / vol_mb:5.1f} volumes, "
              f"peak {peak / 1e6:9.0f} MB = {peak / 1e6 / vol_mb:5.1f} volumes, step {a.elapsed_time(b):8.1f} ms", flush=True)


if __name__ == "__main__":
    memory() if "--memory" in sys.argv[1:] else timings()

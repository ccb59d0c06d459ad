#!/usr/bin/env python3
"""The hourglass close (stereoanywhere_amd.diffops.volume_close: csrc/volume_close.hip) beside the
reference's torch composition on the same GPU: InstanceNorm3d -> LeakyReLU (-> DoubleFeatureAtt's
broadcast gate, F.interpolate and multiply, submodule.py:128-140), gate-less and gated, at the bench
shape's full-resolution volume and its half-resolution one.  Forward (no grad), the backward's launches
alone, and forward + backward through autograd: time per call (20 calls between two events after a
warm-up), the ratio to torch, and TB/s of the bytes model (3 volume passes forward, 5 backward) as a
fraction of the 6.3 TB/s this project measures for HBM.  Inputs rotate over several volumes so that
each call's arrive from HBM, not from the 256 MiB Infinity Cache.

    python scripts/bench_volume_close.py            the timing table
    python scripts/bench_volume_close.py --memory   torch.cuda.max_memory_allocated of one forward + backward of
                                                    diffops.hourglass_forward against blocks.Hourglass's torch
                                                    path at 1 x 8 x 240 x 136 x 240"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from stereoanywhere_amd import blocks, diffops, ops  # noqa: E402

HBM = 6.3   # TB/s achievable on an MI355X
SHAPES = ((4, 8, 240, 136, 240), (4, 16, 120, 68, 120))


def measure(fn, reps=20):
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


def torch_close(x, gl=None, gr=None):
    """BasicConv's norm + act and DoubleFeatureAtt.forward's gate, as the reference composes them."""
    a = F.leaky_relu(F.instance_norm(x), 0.01)
    if gl is None:
        return a
    g = gl.unsqueeze(2) * gr.permute(0, 1, 3, 2).unsqueeze(4)
    g = F.interpolate(g, size=a.shape[2:], mode="trilinear", align_corners=True)
    return g * a


def timings():
    d = torch.device("cuda", 0)
    print("hourglass close: HIP / torch composition in microseconds per call; bytes model 3 volume passes "
          "forward, 5 backward", flush=True)
    print(f"  {'case':<34s} {'HIP us':>9s} {'torch us':>10s} {'ratio':>7s} {'MB model':>9s} {'HIP TB/s':>9s} {'of 6.3':>7s}")
    for shape in SHAPES:
        B, C, D, H, W = shape
        gen = torch.Generator(device=d).manual_seed(0)
        vol_mb = B * C * D * H * W * 4 / 1e6
        ROT = max(2, int(640 / vol_mb) + 1)
        xs = [torch.randn(shape, device=d, generator=gen) for _ in range(ROT)]
        gs = [torch.randn(shape, device=d, generator=gen) for _ in range(ROT)]
        gl = torch.sigmoid(torch.randn(B, C, H, W, device=d, generator=gen))
        gr = torch.sigmoid(torch.randn(B, C, H, D, device=d, generator=gen))
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % ROT
            return xs[turn[0]], gs[turn[0]]

        def line(what, hip_us, torch_us, mb):
            tbs = mb / hip_us   # MB / us = TB/s
            print(f"  {what:<34s} {hip_us:9.1f} {torch_us:10.1f} {torch_us / hip_us:7.2f} {mb:9.1f} {tbs:9.2f} "
                  f"{tbs / HBM:7.2f}", flush=True)

        print(f" volume {'x'.join(map(str, shape))} ({vol_mb:.0f} MB, {ROT} in rotation)", flush=True)
        for gated in (False, True):
            maps = (gl, gr) if gated else (None, None)
            tag = "gated" if gated else "gate-less"
            with torch.no_grad():
                hip_f = measure(lambda: diffops.volume_close(nxt()[0], *maps))
                ref_f = measure(lambda: torch_close(nxt()[0], *maps))
            line(f"{tag} forward", hip_f, ref_f, 3 * vol_mb)
            mean, rstd = ops.volume_close_stats(xs[0])   # (the backward's time does not depend on their values)

            def hip_bwd():
                x, g = nxt()
                return ops.volume_close_backward(g, x, mean, rstd, *maps, 0.01, True, gated, gated)

            def fb(close, wrt_maps):
                x, g = nxt()
                leaves = [x.requires_grad_(True)] + ([m.requires_grad_(True) for m in maps] if wrt_maps else [])
                grads = torch.autograd.grad(close(x, *maps), leaves, g)
                for t in leaves:
                    t.requires_grad_(False)
                return grads

            hip_fb = measure(lambda: fb(diffops.volume_close, gated))
            ref_fb = measure(lambda: fb(torch_close, gated))
            with torch.enable_grad():
                def grad_fwd(close):
                    x = nxt()[0].requires_grad_(True)
                    out = close(x, *maps)
                    x.requires_grad_(False)
                    return out
                ref_gf = measure(lambda: grad_fwd(torch_close))
            hip_b = measure(hip_bwd)
            line(f"{tag} backward (launches alone)", hip_b, ref_fb - ref_gf, 5 * vol_mb)
            line(f"{tag} forward + backward (autograd)", hip_fb, ref_fb, 8 * vol_mb)
        del xs, gs


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
    for name, closes in (("torch path (closes=None)", None), ("HIP closes (closes='hip')", "hip")):
        for step in range(2):   # the second step is the one reported: the first also holds MIOpen's workspaces' search
            hg.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = hg(x, fl, fr, closes=closes)
            held = torch.cuda.memory_allocated() - base
            (out * g).sum().backward()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            del out
        print(f"  {name:<28s} held after the forward {held / 1e6:9.0f} MB = {held / 1e6 / vol_mb:5.1f} volumes, "
              f"peak {peak / 1e6:9.0f} MB = {peak / 1e6 / vol_mb:5.1f} volumes", flush=True)


if __name__ == "__main__":
    memory() if "--memory" in sys.argv[1:] else timings()

#!/usr/bin/env python3
"""The hourglass's up-cat joins (stereoanywhere_amd.diffops.upcat_conv: csrc/conv3d_fused.hip forward,
csrc/upcat_backward.hip backward) beside torch's interpolate + cat + conv3d on the same GPU, at the bench
shape's final join, 4 x (8 | 16 -> 8) x 240 x 136 x 240 <- 120 x 68 x 120, and its half-resolution one,
4 x (16 | 32 -> 16) x 120 x 68 x 120 <- 60 x 34 x 60.  Forward (no grad), the backward's launches alone
(every gradient, and without the skip volume's as at the final join) and forward + backward through
autograd: time per call (20 calls between two events after a warm-up), the ratio to torch, and TB/s of the
bytes model as a fraction of the 6.3 TB/s this project measures for HBM.  Inputs rotate over several
volumes so that each call's arrive from HBM, not from the 256 MiB Infinity Cache.

Bytes model, in volumes' bytes (a, u, out = g, p = dp [B,Cout,low]): forward a + u + 2 p + out; backward
g + dp (the adjoint) + a + g + da (the skip pass) + u + dp + du (the low pass); without da the skip pass is
a + g.

    python scripts/bench_upcat_conv.py            the timing table
    python scripts/bench_upcat_conv.py --memory   held and peak memory of one forward + backward of
                                                  blocks.Hourglass at 1 x 8 x 240 x 136 x 240 with closes="hip"
                                                  alone and with joins="hip" added"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from stereoanywhere_amd import blocks, diffops, ops  # noqa: E402

HBM = 6.3   # TB/s achievable on an MI355X
# (B, (Ca, Cu, Cout), low_first, full, low)
CASES = ((4, (8, 16, 8), False, (240, 136, 240), (120, 68, 120)),
         (4, (16, 32, 16), True, (120, 68, 120), (60, 34, 60)))


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


def torch_join(skip, low, weight, low_first):
    up = F.interpolate(low, size=skip.shape[2:], mode="trilinear", align_corners=True)
    return F.conv3d(torch.cat((up, skip) if low_first else (skip, up), 1), weight)


def timings():
    d = torch.device("cuda", 0)
    print("up-cat conv: HIP / torch interpolate + cat + conv3d in microseconds per call", flush=True)
    print(f"  {'case':<40s} {'HIP us':>9s} {'torch us':>10s} {'ratio':>7s} {'MB model':>9s} {'HIP TB/s':>9s} {'of 6.3':>7s}")
    for B, (ca, cu, cout), low_first, full, low in CASES:
        gen = torch.Generator(device=d).manual_seed(0)
        n, nl = full[0] * full[1] * full[2], low[0] * low[1] * low[2]
        a_mb, u_mb, g_mb, p_mb = (B * c * m * 4 / 1e6 for c, m in ((ca, n), (cu, nl), (cout, n), (cout, nl)))
        ROT = max(2, int(640 / (a_mb + u_mb)) + 1)
        sets = [(torch.randn((B, ca) + full, device=d, generator=gen), torch.randn((B, cu) + low, device=d, generator=gen),
                 torch.randn((B, cout) + full, device=d, generator=gen)) for _ in range(ROT)]
        weight = torch.randn((cout, ca + cu, 1, 1, 1), device=d, generator=gen) * (2.0 / (ca + cu)) ** 0.5
        w_a, w_u = diffops._upcat_weights(weight, ca, low_first)
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % ROT
            return sets[turn[0]]

        def line(what, hip_us, torch_us, mb):
            tbs = mb / hip_us   # MB / us = TB/s
            print(f"  {what:<40s} {hip_us:9.1f} {torch_us:10.1f} {torch_us / hip_us:7.2f} {mb:9.1f} {tbs:9.2f} "
                  f"{tbs / HBM:7.2f}", flush=True)

        print(f" join {B} x ({ca} | {cu} -> {cout}) x {'x'.join(map(str, full))} <- {'x'.join(map(str, low))} "
              f"(a {a_mb:.0f} MB, u {u_mb:.0f} MB, out {g_mb:.0f} MB; {ROT} in rotation)", flush=True)
        with torch.no_grad():
            hip_f = measure(lambda: diffops.upcat_conv(*nxt()[:2], weight, low_first))
            ref_f = measure(lambda: torch_join(*nxt()[:2], weight, low_first))
        line("forward", hip_f, ref_f, a_mb + u_mb + 2 * p_mb + g_mb)

        def hip_bwd(need_skip):
            skip, lowv, g = nxt()
            dp = ops.trilinear_up_adjoint(g, low)
            return (ops.conv3d_pointwise_backward(skip, g, w_a, need_skip, True),
                    ops.conv3d_pointwise_backward(lowv, dp, w_u, True, True))

        def adjoint_alone():
            return ops.trilinear_up_adjoint(nxt()[2], low)

        def fb(join, need_skip):
            skip, lowv, g = nxt()
            leaves = ([skip.requires_grad_(True)] if need_skip else []) + [lowv.requires_grad_(True),
                                                                          weight.requires_grad_(True)]
            grads = torch.autograd.grad(join(skip, lowv, weight, low_first), leaves, g)
            for t in leaves:
                t.requires_grad_(False)
            return grads

        def grad_fwd(join, need_skip):
            skip, lowv, _ = nxt()
            leaves = ([skip.requires_grad_(True)] if need_skip else []) + [lowv.requires_grad_(True),
                                                                          weight.requires_grad_(True)]
            out = join(skip, lowv, weight, low_first)
            for t in leaves:
                t.requires_grad_(False)
            return out

        line("up-sampling adjoint alone", measure(adjoint_alone), float("nan"), g_mb + p_mb)
        for need_skip, tag in ((True, "every gradient"), (False, "no skip gradient")):
            mb_b = g_mb + p_mb + a_mb + g_mb + (a_mb if need_skip else 0.0) + 2 * u_mb + p_mb
            hip_fb = measure(lambda: fb(diffops.upcat_conv, need_skip))
            ref_fb = measure(lambda: fb(torch_join, need_skip))
            ref_gf = measure(lambda: grad_fwd(torch_join, need_skip))
            line(f"backward, {tag} (launches alone)", measure(lambda: hip_bwd(need_skip)), ref_fb - ref_gf, mb_b)
            line(f"forward + backward, {tag} (autograd)", hip_fb, ref_fb, a_mb + u_mb + 2 * p_mb + g_mb + mb_b)
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
    for name, joins in (("closes='hip'", None), ("closes='hip', joins='hip'", "hip")):
        for step in range(2):   # the second step is the one reported: the first also holds MIOpen's workspaces' search
            hg.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = hg(x, fl, fr, closes="hip", joins=joins)
            held = torch.cuda.memory_allocated() - base
            (out * g).sum().backward()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            del out
        print(f"  {name:<28s} held after the forward {held / 1e6:9.0f} MB = {held / 1e6 / vol_mb:5.1f} volumes, "
              f"peak {peak / 1e6:9.0f} MB = {peak / 1e6 / vol_mb:5.1f} volumes", flush=True)


if __name__ == "__main__":
    memory() if "--memory" in sys.argv[1:] else timings()

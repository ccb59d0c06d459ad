#!/usr/bin/env python3
"""The three backward ops of the correlation plug-in (ops.corr_lookup_backward, ops.pyramid_backward,
ops.corr_volume_backward), per-call time beside their bytes / flops models, and torch's own autograd
of the reference formulation (einsum / sqrt(C), avg_pool2d, grid_sample) on the same GPU.

    python scripts/bench_corr_backward.py [B C H W]   (default 4 256 136 240: cfg2 at 1/4 resolution,
                                                       4 levels of radius 4)"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from stereoanywhere_amd import ops  # noqa: E402

L, R = 4, 4


def timeit(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000 / reps


def torch_taps(f2, f3, cx):
    """The reference formulation (corr.py:76-132 of the reference) in torch ops."""
    B, C, H, W1 = f2.shape
    W2 = f3.shape[3]
    level = (torch.einsum("aijk,aijh->ajkh", f2, f3) / torch.sqrt(torch.tensor(float(C)))).reshape(B * H * W1, 1, 1, W2)
    x = cx.permute(0, 2, 3, 1).reshape(B * H * W1, 1, 1, 1)
    dx = torch.linspace(-R, R, 2 * R + 1, device=f2.device).view(1, 1, 2 * R + 1, 1)
    out = []
    for l in range(L):
        xg = 2 * (dx + x / 2 ** l) / (level.shape[-1] - 1) - 1
        out.append(F.grid_sample(level, torch.cat([xg, torch.zeros_like(xg)], dim=-1), align_corners=True)
                   .view(B, H, W1, -1))
        level = F.avg_pool2d(level, [1, 2], stride=[1, 2])
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2)


def main():
    d = torch.device("cuda", 0)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B, C, H, W = (int(v) for v in (args[:4] if len(args) >= 4 else (4, 256, 136, 240)))
    gen = torch.Generator(device=d).manual_seed(0)
    disp = F.interpolate(torch.rand(B, 1, H // 8 + 1, W // 8 + 1, device=d, generator=gen), size=(H, W),
                         mode="bilinear", align_corners=True) * (0.4 * W) + 0.05 * W
    cx = (torch.arange(W, device=d, dtype=torch.float32).view(1, 1, 1, W) - disp).contiguous()
    f2, f3 = torch.randn(B, C, H, W, device=d), torch.randn(B, C, H, W, device=d)
    K = 2 * R + 1
    gout = torch.randn(B, L * K, H, W, device=d)
    rs, _, wids = ops.pyramid_geometry(W, L)
    npix = B * H * W
    gpyr = torch.empty(npix, rs, device=d)
    gvol = torch.empty(npix, W, device=d)
    t_lk = timeit(lambda: ops.corr_lookup_backward(gout, cx, W, L, R, out=gpyr))
    t_py = timeit(lambda: ops.pyramid_backward(gpyr, W, L, out=gvol))
    t_vo = timeit(lambda: ops.corr_volume_backward(gvol, f2, f3))
    b_lk = 4.0 * npix * (L * K + 1 + rs)                      # taps' gradients + coordinate in, whole rows out
    b_py = 4.0 * npix * (sum(wids) + W)                       # every level cell in, level 0 out
    b_vo = 4.0 * (2 * npix * W + 4 * B * C * H * W)           # the volume's gradient per GEMM, 2 maps in, 2 out
    fl_vo = 2 * 2.0 * B * H * C * W * W
    print(f"corr backward B{B} C{C} {H}x{W}, {L} levels of radius {R}:", flush=True)
    print(f"  lookup backward   {t_lk:8.1f} us  ({b_lk / 1e6:.0f} MB model, {b_lk / t_lk / 1e6:.2f} TB/s)", flush=True)
    print(f"  pyramid backward  {t_py:8.1f} us  ({b_py / 1e6:.0f} MB model, {b_py / t_py / 1e6:.2f} TB/s)", flush=True)
    print(f"  volume backward   {t_vo:8.1f} us  ({b_vo / 1e6:.0f} MB model, {b_vo / t_vo / 1e6:.2f} TB/s; "
          f"{fl_vo / 1e9:.1f} GFLOP, {fl_vo / t_vo / 1e6:.1f} TFLOP/s)", flush=True)
    print(f"  sum               {t_lk + t_py + t_vo:8.1f} us", flush=True)
    del gpyr, gvol
    a2, a3 = f2.clone().requires_grad_(), f3.clone().requires_grad_()
    taps = torch_taps(a2, a3, cx)
    t_th = timeit(lambda: torch.autograd.grad(taps, (a2, a3), gout, retain_graph=True), reps=3)
    print(f"  torch autograd of einsum / avg_pool2d / grid_sample (one lookup): {t_th:8.1f} us", flush=True)


if __name__ == "__main__":
    main()

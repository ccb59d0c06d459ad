#!/usr/bin/env python3
"""Forward + backward of the differentiable soft-argmin / confidence and convex up-sampling
(stereoanywhere_amd.diffops) beside torch's own autograd of the same formulas in torch ops
(tests/diffops_ref.py, the restatement the GPU tests use as their reference) on the same GPU: time
per forward + backward (10 calls between two events after a warm-up) and
torch.cuda.max_memory_allocated over them, with the byte models.

    python scripts/bench_diffops_backward.py [B H W]   (default 4 136 240: cfg2 at 1/4 resolution;
                                                        two [B,1,H,W,W] volumes; up-sampling factor 4)"""
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import diffops_ref as ref  # noqa: E402
from stereoanywhere_amd import diffops  # noqa: E402


def measure(fn, reps=10):
    """(us per call, peak bytes allocated above what was held before the calls)"""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000 / reps, torch.cuda.max_memory_allocated() - base


def torch_maps(vd, vc):
    """The four maps by the repository's torch restatement of the formulas (tests/diffops_ref.py)."""
    return (ref.left_disparity(vd[:, 0])[:, None], ref.right_disparity(vd[:, 0])[:, None],
            ref.left_confidence(vc[:, 0])[:, None], ref.right_confidence(vc[:, 0])[:, None])


def torch_upflow(flow, mask):
    return ref.convex_upflow(flow, mask, 4)


def fwd_bwd(fn, inputs, weights):
    def run():
        outs = fn(*inputs)
        outs = outs if isinstance(outs, tuple) else (outs,)
        torch.autograd.grad(outs, inputs, weights)
    return run


def main():
    d = torch.device("cuda", 0)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B, H, W = (int(v) for v in (args[:3] if len(args) >= 3 else (4, 136, 240)))
    vd = (4.0 * torch.randn(B, 1, H, W, W, device=d)).requires_grad_()
    vc = (4.0 * torch.randn(B, 1, H, W, W, device=d)).requires_grad_()
    gw = tuple(torch.randn(B, 1, H, W, device=d) for _ in range(4))
    vol = 4.0 * B * H * W * W
    print(f"soft-argmin + confidence, two volumes B{B} {H}x{W}x{W} ({vol / 1e6:.0f} MB each):", flush=True)
    t, m = measure(fwd_bwd(diffops.softargmin_conf, (vd, vc), gw))
    # forward: each volume read once; backward: read twice, gradient written once
    model = 2 * 4 * vol
    print(f"  HIP forward + backward   {t:9.1f} us  peak {m / 1e6:8.0f} MB above the inputs "
          f"({model / 1e6:.0f} MB traffic model, {model / t / 1e6:.2f} TB/s; 2 gradients = {2 * vol / 1e6:.0f} MB)",
          flush=True)
    t, m = measure(fwd_bwd(torch_maps, (vd, vc), gw))
    print(f"  torch autograd           {t:9.1f} us  peak {m / 1e6:8.0f} MB above the inputs", flush=True)
    del vd, vc, gw
    torch.cuda.empty_cache()

    flow = (10.0 * torch.randn(B, 1, H, W, device=d)).requires_grad_()
    mask = torch.randn(B, 144, H, W, device=d).requires_grad_()
    gu = (torch.randn(B, 1, 4 * H, 4 * W, device=d),)
    mb = 4.0 * B * 144 * H * W
    print(f"convex up-sampling B{B} {H}x{W}, factor 4 (mask {mb / 1e6:.0f} MB):", flush=True)
    t, m = measure(fwd_bwd(diffops.convex_upflow, (flow, mask), gu))
    # forward: mask read, output written; backward: mask read by each of the two kernels, grad_mask written
    model = 4 * mb + 3 * mb / 9
    print(f"  HIP forward + backward   {t:9.1f} us  peak {m / 1e6:8.0f} MB above the inputs "
          f"({model / 1e6:.0f} MB traffic model, {model / t / 1e6:.2f} TB/s; grad_mask = {mb / 1e6:.0f} MB)", flush=True)
    t, m = measure(fwd_bwd(torch_upflow, (flow, mask), gu))
    print(f"  torch autograd           {t:9.1f} us  peak {m / 1e6:8.0f} MB above the inputs", flush=True)


if __name__ == "__main__":
    main()

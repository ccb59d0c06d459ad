#!/usr/bin/env python3
"""Forward + backward of the differentiable softlrc_conf and weighted_lsq (stereoanywhere_amd.diffops)
beside torch's own autograd of the same formulas in torch ops (tests/lsq_lrc_ref.py, the restatement
the GPU tests use as their reference: grid_sample, torch.quantile, boolean indexing and
torch.linalg.lstsq per sample, as the reference model runs them) on the same GPU: time per forward +
backward (10 calls between two events after a warm-up) and torch.cuda.max_memory_allocated over them.
The softlrc backward is also timed without its gather (confidence gradients only) to price the O(W)
scan.

    python scripts/bench_lsq_lrc_backward.py [B H W]   (default 4 136 240: cfg2 at 1/4 resolution, the
                                                        joint L + R maps 2 x H x W per sample)"""
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lsq_lrc_ref as ref  # noqa: E402
from stereoanywhere_amd import diffops, ops  # noqa: E402


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


def fwd_bwd(fn, inputs, weights):
    def run():
        torch.autograd.grad(fn(*inputs), inputs, weights)
    return run


def torch_lsq(mde, disp, conf):
    B = mde.shape[0]
    return ref.weighted_lsq(mde.reshape(B, -1), disp.reshape(B, -1), conf.reshape(B, -1), torch.float32)


def hip_lsq(mde, disp, conf):
    scale, shift = diffops.weighted_lsq(mde, disp, conf)
    return scale.flatten(), shift.flatten()


def line(what, t, m):
    print(f"  {what:<34s} {t:9.1f} us  peak {m / 1e6:7.2f} MB above the inputs", flush=True)


def main():
    d = torch.device("cuda", 0)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B, H, W = (int(v) for v in (args[:3] if len(args) >= 3 else (4, 136, 240)))
    gen = torch.Generator(device=d).manual_seed(0)
    # disparities as the model's coarse maps: tens of pixels, some negative
    d2, d3 = ((0.15 * W * torch.randn(B, 1, H, W, device=d, generator=gen) + 0.1 * W).requires_grad_() for _ in range(2))
    c2, c3 = (torch.rand(B, 1, H, W, device=d, generator=gen).requires_grad_() for _ in range(2))
    gw = tuple(torch.randn(B, 1, H, W, device=d, generator=gen) for _ in range(2))
    mb = 4.0 * B * H * W / 1e6
    print(f"softlrc_conf B{B} {H}x{W} (a map {mb:.2f} MB; 4 inputs, 2 outputs):", flush=True)
    line("HIP forward + backward", *measure(fwd_bwd(diffops.softlrc_conf, (d2, d3, c2, c3), gw)))
    line("torch autograd", *measure(fwd_bwd(lambda *a: ref.softlrc(*a), (d2, d3, c2, c3), gw)))
    raw = [t.detach() for t in (d2, d3, c2, c3)]
    line("HIP forward alone", *measure(lambda: ops.softlrc(*raw, 1.0)))
    line("HIP backward, all four gradients", *measure(lambda: ops.softlrc_backward(*raw, 1.0, *gw, True, True, True, True)))
    line("HIP backward without the gather", *measure(lambda: ops.softlrc_backward(*raw, 1.0, *gw, False, False, True, True)))
    print(f"  (the gather: {2 * B * H * W} target pixels x up to 3 rows x {W} source pixels = "
          f"{2 * B * H * W * 2 * W / 1e6:.0f} M tap tests at 2 rows)", flush=True)

    mde = (3.0 * torch.randn(B, 2, H, W, device=d, generator=gen)).requires_grad_()
    disp = torch.cat([d2, d3], 1).detach().requires_grad_()
    conf = torch.rand(B, 2, H, W, device=d, generator=gen).requires_grad_()
    gs = tuple(torch.randn(B, device=d, generator=gen) for _ in range(2))
    print(f"weighted_lsq B{B}, {2 * H * W} elements per sample (3 maps of {2 * mb:.2f} MB):", flush=True)
    line("HIP forward + backward", *measure(fwd_bwd(hip_lsq, (mde, disp, conf), gs)))
    line("torch autograd", *measure(fwd_bwd(torch_lsq, (mde, disp, conf), gs)))
    raw = [t.detach().reshape(B, -1) for t in (mde, disp, conf)]
    line("HIP forward alone (inference)", *measure(lambda: ops.weighted_lsq(*raw)))
    line("HIP forward alone (with record)", *measure(lambda: ops.weighted_lsq_stats(*raw)))
    sc, sh, rec = ops.weighted_lsq_stats(*raw)
    line("HIP backward alone", *measure(lambda: ops.weighted_lsq_backward(*raw, sc, sh, rec, *gs)))


if __name__ == "__main__":
    main()

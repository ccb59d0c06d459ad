#!/usr/bin/env python3
"""The fused training loss (stereoanywhere_amd.losses.training_loss) beside torch's own autograd of the
same block in torch ops (tests/losses_ref.py, the restatement the GPU tests use as their reference:
boolean-mask gathers, padded differences, the isnan checks on the host, as train.py runs them) on the
same GPU: the fine-tuning shape, 22 full-resolution predictions plus the three coarse entries of both
sides, every term on.  Time per call (10 calls between two events after a warm-up) and
torch.cuda.max_memory_allocated over them, forward alone and forward + backward.

    python scripts/bench_losses.py [B H W N]   (default 4 544 960 22)"""
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import losses_ref as ref  # noqa: E402
from stereoanywhere_amd import losses, ops  # noqa: E402

ARGS = dict(maxdisp=192.0, lrc_th=1.0, normal_gain=10, use_normal_loss=True, use_normal_loss_on_coarse=True,
            use_border_mask=True)


def measure(fn, reps=10):
    """(ms per call, peak bytes allocated above what was held before the calls)"""
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
    return a.elapsed_time(b) / reps, torch.cuda.max_memory_allocated() - base


def torch_loss(outputs, data, targets):
    pred_disps, pred_confs, disps0, disps1, confs0, confs1 = outputs
    gain = data["gt"].shape[-1] / ARGS["normal_gain"]
    kw = dict(maxdisp=ARGS["maxdisp"], gain=gain, lrc_th=ARGS["lrc_th"])
    total = ref.loss_terms(ref.sequence_maps(pred_disps, use_normal_loss=True), data["gt"], data["validgt"],
                           target=targets[0], border="none", **kw)[0]
    total = total + ref.loss_terms(ref.coarse_maps(disps0, confs0, side="left", use_normal_loss_on_coarse=True),
                                   data["gt"], data["validgt"], target=targets[0], border="left", **kw)[0]
    return total + ref.loss_terms(ref.coarse_maps(disps1, confs1, side="right", use_normal_loss_on_coarse=True),
                                  data["gt_right"], data["validgt_right"], target=targets[1], border="right", **kw)[0]


def line(what, t, m):
    print(f"  {what:<28s} {t:9.3f} ms  peak {m / 1e6:9.1f} MB above the inputs", flush=True)


def main():
    d = torch.device("cuda", 0)
    args = [int(a) for a in sys.argv[1:]]
    B, H, W, n = args if len(args) == 4 else (4, 544, 960, 22)
    gen = torch.Generator(device=d).manual_seed(0)
    rand = lambda lo, hi: lo + (hi - lo) * torch.rand(B, 1, H, W, device=d, generator=gen)
    data = {}
    for side in ("", "_right"):
        data["gt" + side] = rand(0.5, 220.0)
        data["validgt" + side] = (rand(0, 1) < 0.8).float()
    data["im2_mono"], data["im3_mono"] = rand(0, 1), rand(0, 1)
    noisy = lambda gt, sign: (sign * (gt + 3.0 * torch.randn(gt.shape, device=d, generator=gen))).requires_grad_()
    outputs = ([noisy(data["gt"], -1) for _ in range(n)], [None] * n,
               [noisy(data["gt"], 1) for _ in range(3)], [noisy(data["gt_right"], 1) for _ in range(3)],
               [rand(0.02, 0.98).requires_grad_() for _ in range(3)], [rand(0.02, 0.98).requires_grad_() for _ in range(3)])
    leaves = [t for group in outputs for t in group if t is not None]
    targets = [ops.mono_normals(data[k], W / ARGS["normal_gain"]) for k in ("im2_mono", "im3_mono")]
    mb = 4.0 * B * H * W / 1e6
    maps = n + 6
    print(f"training loss B{B} {H}x{W}, {n} predictions + 6 coarse maps + 6 confidences (a map {mb:.2f} MB):", flush=True)
    hip = lambda: losses.training_loss(outputs, data, ARGS)[0]
    with torch.no_grad():
        hip_f = measure(hip)
        torch_f = measure(lambda: torch_loss(outputs, data, targets))
    line("HIP forward", *hip_f)
    line("torch forward", *torch_f)
    hip_fb = measure(lambda: torch.autograd.grad(hip(), leaves))
    torch_fb = measure(lambda: torch.autograd.grad(torch_loss(outputs, data, targets), leaves))
    line("HIP forward + backward", *hip_fb)
    line("torch forward + backward", *torch_fb)
    line("HIP backward (difference)", hip_fb[0] - hip_f[0], 0)
    a, b = float(hip().detach()), float(torch_loss(outputs, data, targets).detach())
    print(f"  totals: HIP {a:.6f}, torch fp32 {b:.6f}", flush=True)
    # bytes model: forward reads every map twice (min / max pass, sums pass) and a confidence once;
    # gt / valid / target once per tile and call; backward reads a map and writes its gradient
    fwd = (2 * maps + 6) * mb + 3 * (2 + 3) * mb
    bwd = (2 * maps + 2 * 6) * mb + 3 * (2 + 3) * mb
    print(f"  bytes model: forward {fwd:.0f} MB ({fwd / hip_f[0] / 1e3:.2f} TB/s at the measured time), backward "
          f"{bwd:.0f} MB ({bwd / max(hip_fb[0] - hip_f[0], 1e-9) / 1e3:.2f} TB/s)", flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The volume stage (stereoanywhere_amd.diffops.volume_stage: csrc/volume_stage.hip) beside the same
stage as a chain of torch element-wise ops on the same GPU, written out below from the formulas of
include/stereoanywhere_hip.h the way the reference's forward composes them (the blend
v (1 - m) + src m from an fp16 mask, the mask volume of the truncation, torch.max(...).item() for
the zeroing): each kind, with and without the truncation, forward; and the truncation's forward +
backward.  Time per call (20 calls between two events after a warm-up) and TB/s of the bytes model:
one volume read, one written, plus the per-pixel maps.

    python scripts/bench_volume_stage.py [B H W]   (default 4 136 240: the bench shape, W1 = W2 = W)"""
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from stereoanywhere_amd import diffops, ops  # noqa: E402
from stereoanywhere_amd.diffops import VolumeCorruption  # noqa: E402

N_MASKS, BIN, ATTEN = 4, 1, 0.9
HBM = 6.3   # TB/s achievable on an MI355X


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


def torch_mask(mde, n, b):
    return ((mde < (b + 1) / n) & (mde >= b / n)).half().unsqueeze(4)


def torch_trunc_mask(disp, conf, atten):
    W = disp.shape[3]
    j = torch.arange(W, device=disp.device, dtype=disp.dtype).view(1, 1, 1, W, 1)
    k = torch.arange(W, device=disp.device, dtype=disp.dtype).view(1, 1, 1, 1, W)
    t = conf.unsqueeze(4)
    return 1 * (1 - t) + t * (torch.sigmoid((j - disp.unsqueeze(4)) - k) * (1 - atten) + atten)


def torch_stage(v, mde, kind, shift, trunc):
    """The torch expression chain of one touched volume (stereoanywhere.py:214-255 restated)."""
    if kind != "none":
        m = torch_mask(mde, N_MASKS, BIN)
        if kind == "roll":
            src = torch.roll(v, shifts=shift, dims=3)
        elif kind == "noise":
            src = v * torch.rand_like(m)
        else:
            W = v.shape[3]
            j = torch.arange(W, device=v.device, dtype=v.dtype).view(1, 1, 1, W, 1)
            k = torch.arange(W, device=v.device, dtype=v.dtype).view(1, 1, 1, 1, W)
            x = j - k
            src = v * (torch.max(v).cpu().item() * torch.exp(-(x ** 2) / 2))
        v = (v * (1 - m) + src * m).detach()
    if trunc is not None:
        v = torch_trunc_mask(*trunc).detach() * v
    return v


def main():
    d = torch.device("cuda", 0)
    args = [int(a) for a in sys.argv[1:]]
    B, H, W = args if len(args) == 3 else (4, 136, 240)
    gen = torch.Generator(device=d).manual_seed(0)
    vol = torch.randn(B, 1, H, W, W, device=d, generator=gen)
    mde = torch.rand(B, 1, H, W, device=d, generator=gen)
    disp = torch.rand(B, 1, H, W, device=d, generator=gen) * (W / 4)
    conf = torch.rand(B, 1, H, W, device=d, generator=gen)
    vol_mb, map_mb = vol.numel() * 4 / 1e6, mde.numel() * 4 / 1e6
    print(f"volume stage B{B} H{H} W1 = W2 = {W} (a volume {vol_mb:.1f} MB, a map {map_mb:.2f} MB); "
          f"HIP / torch chain in microseconds per call", flush=True)
    print(f"  {'case':<22s} {'HIP us':>9s} {'torch us':>10s} {'ratio':>7s} {'MB model':>9s} {'HIP TB/s':>9s} {'of 6.3':>7s}")
    # A volume of the default shape fits in the 256 MiB Infinity Cache, so calls on one volume are
    # partly served from it.  The HIP and torch columns therefore rotate over ROT volumes (more than
    # the cache holds between two uses of one of them), as a training step's volume arrives from HBM.
    ROT = max(2, int(640 / vol_mb) + 1)
    vols = [vol] + [torch.randn_like(vol) for _ in range(ROT - 1)]
    turn = [0]

    def nxt():
        turn[0] = (turn[0] + 1) % ROT
        return vols[turn[0]]

    def line(what, hip_us, torch_us, mb):
        tbs = mb / hip_us   # MB / us = TB/s
        print(f"  {what:<22s} {hip_us:9.1f} {torch_us:10.1f} {torch_us / hip_us:7.1f} {mb:9.1f} {tbs:9.2f} {tbs / HBM:7.2f}",
              flush=True)

    with torch.no_grad():
        for kind in ("none", "roll", "noise", "zero"):
            for trunc in (None, (disp, conf, ATTEN)):
                if kind == "none" and trunc is None:
                    continue
                plan = None if kind == "none" else VolumeCorruption("stereo", kind, BIN, W // 3 if kind == "roll" else 0)
                hip = measure(lambda: diffops.volume_stage(nxt(), vol, mde, plan, trunc, n_masks=N_MASKS))
                ref = measure(lambda: torch_stage(nxt(), mde, kind, W // 3, trunc))
                if kind == "none":   # the same call on one volume, for the cache's share
                    warm = measure(lambda: diffops.volume_stage(vol, vol, mde, plan, trunc, n_masks=N_MASKS))
                    print(f"  (none + trunc on one volume every call: {warm:.1f} us, Infinity-Cache assisted)", flush=True)
                # one read, one write, the maps it reads; "zero" reads the volume once more for its maximum;
                # "noise" also writes and reads the drawn fp16 map
                maps = (kind != "none") + 2 * (trunc is not None) + (kind == "noise")
                mb = 2 * vol_mb + maps * map_mb + (vol_mb if kind == "zero" else 0)
                line(f"{kind}{' + trunc' if trunc else ''}", hip, ref, mb)
    # the differentiable route: truncation forward + backward with respect to the volume
    leaf = vol.clone().requires_grad_()
    g = torch.randn_like(vol)
    trunc = (disp, conf, ATTEN)
    hip_f = measure(lambda: diffops.truncate_volume(leaf, *trunc))
    ref_f = measure(lambda: torch_stage(leaf, mde, "none", 0, trunc))
    hip_fb = measure(lambda: torch.autograd.grad(diffops.truncate_volume(leaf, *trunc), leaf, g))
    ref_fb = measure(lambda: torch.autograd.grad(torch_stage(leaf, mde, "none", 0, trunc), leaf, g))
    mb = 2 * vol_mb + 2 * map_mb
    line("trunc fwd (grad mode)", hip_f, ref_f, mb)
    line("trunc fwd + bwd", hip_fb, ref_fb, 2 * mb)
    line("trunc bwd (difference)", hip_fb - hip_f, ref_fb - ref_f, mb)
    # the adjoint's launch alone, without autograd's round trip through Python and the engine's thread
    # (which, not the kernel, bounds the HIP forward + backward above); torch's is its one multiply
    mask = torch_trunc_mask(*trunc)
    line("trunc bwd launch alone", measure(lambda: ops.volume_truncate_backward(nxt(), disp, conf, ATTEN)),
         measure(lambda: mask * nxt()), mb)
    del mask
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = diffops.truncate_volume(leaf, *trunc)
    hip_held = torch.cuda.memory_allocated() - base
    del out
    base = torch.cuda.memory_allocated()
    out = torch_stage(leaf, mde, "none", 0, trunc)
    ref_held = torch.cuda.memory_allocated() - base
    print(f"  held for the backward besides the inputs: HIP {hip_held / 1e6:.1f} MB (the output), "
          f"torch {ref_held / 1e6:.1f} MB (the output and the mask volume)", flush=True)


if __name__ == "__main__":
    main()

"""Float64 CPU reference of the hourglass's up-cat joins (diffops.upcat_conv, csrc/upcat_backward.hip): the
composition ``F.interpolate(trilinear, align_corners=True)`` -> ``cat`` -> ``F.conv3d`` with autograd's
gradients, and the seeded cases the GPU tests share.  Independent of the HIP kernels and their wrappers;
tests/test_upcat_conv_ref_cpu.py pins it to blocks.Hourglass's two joins and to hourglass_ref.upcat."""
import functools

import torch
import torch.nn.functional as F

B = 2
# (full, low): test_gpu_hourglass_ref.UPCAT_SHAPES (full tiles at exactly half; three W tiles with a
# 2-column tail and odd D; a factor above 2, inexact scales and W % 4 != 0; the smallest volume, every tap
# into one cell) plus one axis of the low branch of length 1 and twelve planes into one
SHAPES = (((8, 12, 64), (4, 6, 32)), ((9, 6, 130), (5, 3, 65)), ((10, 7, 67), (3, 2, 20)), ((2, 2, 2), (1, 1, 1)),
          ((5, 4, 6), (3, 1, 3)), ((12, 4, 8), (1, 2, 4)))
# ((Ca, Cu, Cout), low_first): final_agg[0] over cat(orig, up) and agg_layers[1][0] over cat(up, down0)
TRIPLES = (((8, 16, 8), False), ((16, 32, 16), True))
GRADS = ("da", "du", "dW", "dp")


def up(low, size):
    return F.interpolate(low, size=tuple(size), mode="trilinear", align_corners=True)


def compose(skip, low, weight, low_first):
    """The join in the inputs' dtype: conv3d(cat((up(low), skip) if low_first else (skip, up(low)), 1), weight)."""
    u = up(low, skip.shape[2:])
    return F.conv3d(torch.cat((u, skip) if low_first else (skip, u), 1), weight)


def split(weight, ca, low_first):
    """The module's [Cout, Ca+Cu, 1, 1, 1] weight -> (w_a [Ca][Cout], w_u [Cu][Cout]), the kernels' layouts."""
    w = weight.reshape(weight.shape[0], -1)
    cu = w.shape[1] - ca
    w_a, w_u = (w[:, cu:], w[:, :cu]) if low_first else (w[:, :ca], w[:, ca:])
    return w_a.t().contiguous(), w_u.t().contiguous()


def evaluate(skip, low, weight, g, low_first, dtype):
    """out and the gradients of sum(out * g) by autograd, in `dtype` on the CPU -> dict(out, da, du, dW, dp);
    dp is the gradient of sum(up(p) * g) with respect to a p [B,Cout,*low size]: the interpolation's
    transpose applied to g."""
    a, u, w = (t.detach().to(dtype, copy=True).requires_grad_(True) for t in (skip, low, weight))
    out = compose(a, u, w, low_first)
    da, du, dW = torch.autograd.grad(out, (a, u, w), g.to(dtype))
    p = torch.zeros((low.shape[0], weight.shape[0]) + tuple(low.shape[2:]), dtype=dtype, requires_grad=True)
    dp, = torch.autograd.grad(up(p, skip.shape[2:]), p, g.to(dtype))
    return dict(out=out.detach(), da=da, du=du, dW=dW, dp=dp)


def metric(got, ref):
    """max |got - ref| / max |ref|."""
    return float((got.double().cpu() - ref.double()).abs().max() / ref.double().abs().max())


def _case(full, low, triple, low_first, seed):
    ca, cu, cout = triple
    gen = torch.Generator().manual_seed(7000 + seed)
    skip = torch.randn((B, ca) + tuple(full), generator=gen, dtype=torch.float32)
    lowv = torch.randn((B, cu) + tuple(low), generator=gen, dtype=torch.float32)
    weight = torch.randn((cout, ca + cu, 1, 1, 1), generator=gen, dtype=torch.float32) * (2.0 / (ca + cu)) ** 0.5
    g = torch.randn((B, cout) + tuple(full), generator=gen, dtype=torch.float32)
    return dict(seed=seed, skip=skip, low=lowv, weight=weight, g=g, low_first=low_first, triple=triple,
                ref=evaluate(skip, lowv, weight, g, low_first, torch.float64),
                f32=evaluate(skip, lowv, weight, g, low_first, torch.float32))


@functools.lru_cache(maxsize=None)
def case(full, low, triple, low_first):
    """One seeded case, built once and shared: the fp32 inputs, the float64 reference (`ref`) and torch's
    fp32 CPU composition (`f32`).  Nobody modifies it.

    The seed is the first whose fp32 CPU composition deviates from float64 by at least half an fp32 ulp of
    the largest value (2^-25 in `metric`) in every gradient (volume_close_ref.case's rule: 4 x a figure
    that happens to be far below half an ulp is no measure of fp32 arithmetic).  The choice is made on the
    CPU from torch's two compositions alone."""
    for seed in range(64):
        c = _case(full, low, triple, low_first, seed)
        if all(metric(c["f32"][k], c["ref"][k]) >= 2.0 ** -25 for k in GRADS):
            return c
    raise AssertionError(f"no representative seed for {full} <- {low}, {triple}")


def allowance(c, key):
    """4 x the deviation of torch's fp32 CPU composition from float64, in `metric`: the kernels make the
    same handful of fp32 roundings per value in another order."""
    return 4.0 * metric(c["f32"][key], c["ref"][key])

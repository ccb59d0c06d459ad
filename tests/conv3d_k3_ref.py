"""float64 reference of diffops.conv3d_k3 (a stride-1, pad-1, bias-free 3x3x3 conv with equal channel counts
and its two gradients), its seeded cases, the scale rule of sa_sample_scale and the dw bound of DESIGN.md 4l.

The reference is ``F.conv3d(x, weight, padding=1)`` in float64 with autograd's gradients.  Cases are built once
per shape (functools.lru_cache) and shared; nobody writes to them."""
import functools

import numpy as np
import torch

F = torch.nn.functional
U = 2.0 ** -24   # unit roundoff of fp32
R_CHAIN = 1024   # products an fp32 MFMA accumulator takes before it goes into float64 (kR of conv3d_backward.hip)
# (R + c) u mag: R u for the fp32 additions of one chain of R products (a chain starts at zero and every later
# partial is float64), 3 terms x 2^-22 = 12 u for the split (each operand is its hi + lo to 2^-22, the dropped
# lo lo term is below 2^-22 of the product), 1 u for the final rounding of the float64 sum to fp32 and 1 u for
# everything done in float64
C_SPLIT = 14

# (C, B, D, H, W)
SHAPES = ((8, 2, 5, 9, 70), (8, 1, 2, 1, 2), (16, 2, 7, 5, 66), (16, 1, 3, 4, 64), (32, 2, 4, 5, 40),
          (32, 1, 9, 6, 33))
PLANES = {(16, 2, 7, 5, 66): 3}   # sa_conv3d_mf_set_planes for this shape: a D-tile seam inside the volume


def conv(x, weight):
    return F.conv3d(x, weight, padding=1)


def grads(x, weight, g):
    """(dx, dw) of sum(conv(x, weight) * g) by autograd, in the tensors' dtype."""
    x, weight = x.detach().clone().requires_grad_(True), weight.detach().clone().requires_grad_(True)
    (conv(x, weight) * g).sum().backward()
    return x.grad, weight.grad


def flipped(weight):
    """The weight whose plain conv is the data gradient: kernel flipped on all three axes, channel roles swapped."""
    return weight.flip(2, 3, 4).transpose(0, 1)


def to_taps(w):
    """The module's [Cout, Cin, 3, 3, 3] -> ops.conv3d's [Cin][27][Cout]."""
    co, ci = w.shape[:2]
    return w.reshape(co, ci, 27).permute(1, 2, 0).contiguous()


def from_taps(w_t):
    ci, _, co = w_t.shape
    return w_t.permute(2, 0, 1).reshape(co, ci, 3, 3, 3).contiguous()


def scale_exponent(amax: float) -> int:
    """k of s = 2^k: max * s in [2^13, 2^14), |k| <= 100; 0 for a zero or non-finite maximum."""
    if amax == 0.0 or not np.isfinite(amax):
        return 0
    _, e = np.frexp(np.float32(amax))   # amax in [2^(e-1), 2^e)
    return int(np.clip(14 - int(e), -100, 100))


def sample_scales(t):
    """[B] float32 scales of a [B, ...] tensor by the rule above (NaN counts as non-finite)."""
    flat = t.detach().reshape(t.shape[0], -1).abs().double().cpu().numpy()
    return np.array([np.ldexp(1.0, scale_exponent(float(row.max()) if not np.isnan(row).any() else np.nan))
                     for row in flat], dtype=np.float32)


def dw_bound(mag):
    return (R_CHAIN + C_SPLIT) * U * mag


@functools.lru_cache(maxsize=None)
def case(C, B, D, H, W):
    """x, g [B,C,D,H,W], weight [C,C,3,3,3] (fp32, CPU) and the float64 out, dx, dw and dw's magnitude
    sum |x| |g| (module layout)."""
    gen = torch.Generator().manual_seed(1000 * C + 100 * B + 10 * D + H + W)
    x = torch.randn(B, C, D, H, W, generator=gen)
    g = torch.randn(B, C, D, H, W, generator=gen)
    weight = torch.randn(C, C, 3, 3, 3, generator=gen) * (2.0 / (27 * C)) ** 0.5
    x64, w64, g64 = x.double(), weight.double(), g.double()
    dx, dw = grads(x64, w64, g64)
    _, mag = grads(x64.abs(), w64, g64.abs())   # the weight gradient is bilinear in (x, g) and free of w
    return dict(x=x, g=g, weight=weight, out=conv(x64, w64), dx=dx, dw=dw, mag=mag)

"""Float64 CPU reference of the hourglass close (csrc/volume_close.hip, diffops.volume_close): the
composition ``F.instance_norm`` -> ``F.leaky_relu`` -> ``* gl[:, :, None] * gr.permute(0, 1, 3, 2)[..., None]``
on a volume [B, C, D = W2, H, W = W1], its gradients from torch autograd, and the seeded cases the GPU
tests share.  Independent of the HIP kernels and their wrappers; tests/test_volume_close_ref_cpu.py pins
it to blocks.BasicConv / blocks.DoubleFeatureAtt and to hourglass_ref.T.

The input builder keeps every normalised value away from the LeakyReLU kink: a cell with |xh| < 1e-3
(float64) is pushed by +-4e-3 / rstd and the volume re-rounded to fp32, at most four times, so that a
kernel's fp32 xh and the reference's float64 xh agree on every sign and no cell has to be left out."""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24   # unit roundoff of float32
SLOPE, EPS = 0.01, 1e-5
# (B, C, D, H, W): odd D and W over one wave with a tail that is no multiple of 4; a narrow row; the
# smallest legal n; more d-steps than a wave's reduction tree and three rounds of 64 lanes
SHAPES = ((2, 2, 5, 3, 70), (1, 8, 4, 2, 9), (1, 2, 1, 2, 3), (1, 1, 33, 2, 130))
KINK, PUSH, ROUNDS = 1e-3, 4e-3, 4


def stats(x, eps=EPS):
    """InstanceNorm3d statistics in x's dtype -> (mean, rstd), [B*C] each (biased variance)."""
    var, mean = torch.var_mean(x, dim=(2, 3, 4), unbiased=False)
    return mean.reshape(-1), torch.rsqrt(var + eps).reshape(-1)


def xhat(x, eps=EPS):
    """The normalised volume in float64."""
    x = x.double()
    B, C = x.shape[:2]
    mean, rstd = (t.reshape(B, C, 1, 1, 1) for t in stats(x, eps))
    return (x - mean) * rstd


def gate(gl, gr):
    return gl[:, :, None] * gr.permute(0, 1, 3, 2)[..., None]


def close(x, gl=None, gr=None, slope=SLOPE, eps=EPS):
    """The close in x's dtype."""
    a = F.leaky_relu(F.instance_norm(x, eps=eps), slope)
    return a if gl is None else a * gl[:, :, None] * gr.permute(0, 1, 3, 2)[..., None]


def build_x(seed, shape, eps=EPS):
    """Seeded normal fp32 volume with every |xh| kept off the kink (module docstring)."""
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    B, C = shape[:2]
    for _ in range(ROUNDS):
        xh = xhat(x, eps)
        near = xh.abs() < KINK
        if not near.any():
            break
        rstd = stats(x.double(), eps)[1].reshape(B, C, 1, 1, 1)
        push = torch.where(xh >= 0, 1.0, -1.0).double() * PUSH / rstd
        x = torch.where(near, x.double() + push, x.double()).float()
    return x


def evaluate(x, g, gl, gr, dtype, slope=SLOPE, eps=EPS):
    """out and the gradients of sum(out * g) by autograd, all in `dtype` on the CPU ->
    dict(mean, rstd, out, dx, dgl, dgr); the gate entries are None without a gate."""
    x = x.detach().to(dtype, copy=True).requires_grad_(True)
    maps = [] if gl is None else [t.detach().to(dtype, copy=True).requires_grad_(True) for t in (gl, gr)]
    out = close(x, *maps, slope=slope, eps=eps)
    grads = torch.autograd.grad(out, [x] + maps, g.to(dtype))
    mean, rstd = stats(x.detach(), eps)
    return dict(mean=mean, rstd=rstd, out=out.detach(), dx=grads[0], dgl=grads[1] if maps else None,
                dgr=grads[2] if maps else None)


def gate_mags(x, g, gl, gr, slope=SLOPE, eps=EPS):
    """The two gate gradients' sums over absolute values (float64): the scale of their rounding bound."""
    ga = (g.double() * F.leaky_relu(xhat(x, eps), slope)).abs()
    return ((ga * gr.double().permute(0, 1, 3, 2)[..., None]).sum(2),                 # [B,C,H,W], D terms
            (ga * gl.double()[:, :, None]).sum(4).permute(0, 1, 3, 2).contiguous())   # [B,C,H,D], W terms


def metric(got, ref):
    """max |got - ref| / max |ref|."""
    return float((got.double().cpu() - ref.double()).abs().max() / ref.double().abs().max())


@functools.lru_cache(maxsize=None)
def case(shape, gated):
    """One seeded case, built once and shared: the fp32 inputs, the float64 reference (`ref`), torch's
    fp32 CPU composition (`f32`) and, gated, the gate gradients' magnitudes.  Nobody modifies it.

    The seed is the first whose fp32 CPU composition deviates from float64 by at least half an fp32 ulp
    of the largest value (2^-25 in `metric`) in out and in dx.  Every fp32 evaluation makes three or four
    roundings per cell, so half an ulp is the least a worst cell can be expected to show; over the dozen
    cells of the smallest shape torch's composition happens to stay well below it for some draws, and
    4 x such a lucky figure is no measure of fp32 arithmetic.  The choice is made on the CPU from torch's
    two compositions alone."""
    for seed in range(64):
        c = _case(shape, gated, seed)
        if all(metric(c["f32"][k], c["ref"][k]) >= 2.0 ** -25 for k in ("out", "dx")):
            return c
    raise AssertionError(f"no representative seed for {shape}")


def _case(shape, gated, seed):
    B, C, D, H, W = shape
    gen = torch.Generator().manual_seed(1000 + seed)
    x = build_x(seed, shape)
    g = torch.randn(shape, generator=gen, dtype=torch.float32)
    gl = gr = None
    if gated:
        gl = torch.sigmoid(torch.randn((B, C, H, W), generator=gen, dtype=torch.float32))
        gr = torch.sigmoid(torch.randn((B, C, H, D), generator=gen, dtype=torch.float32))
    c = dict(seed=seed, x=x, g=g, gl=gl, gr=gr, ref=evaluate(x, g, gl, gr, torch.float64), f32=evaluate(x, g, gl, gr, torch.float32))
    if gated:
        c["mag_l"], c["mag_r"] = gate_mags(x, g, gl, gr)
    return c


def allowance(c, key):
    """4 x the deviation of torch's fp32 CPU composition from float64, in `metric`: the kernel makes the
    same handful of fp32 roundings per cell in another order."""
    return 4.0 * metric(c["f32"][key], c["ref"][key])

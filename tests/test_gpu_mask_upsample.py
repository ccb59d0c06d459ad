"""sa_mask_upsample (csrc/mask_upsample.hip): the mask head's 1x1 conv, the softmax over the nine
neighbours and the convex up-sampling of factor 4 in one kernel, against a float64 conv -> softmax ->
weighted sum from the same fp32 inputs, and against the unfused pair sa_conv1x1 + sa_convex_upsample.

Bound per output.  The logits z carry the error that tests/test_gpu_conv1x1.py gates on sa_conv1x1's
output, eps = 2e-6 * max|z64|.  A softmax whose logits move by at most +-eps has every weight within a
factor e^(+-2 eps) of the exact one, and the output is a convex combination of the nine neighbours
v_k = 4 flow (zero-padded), so it moves by at most (e^(2 eps) - 1) * R with R = max_k v_k - min_k v_k.
The fp32 evaluation (max, 9 exp, sum, reciprocal, 9 multiply-adds of terms below M = max_k |v_k|) is
allowed 64 * 2^-24 * M:

    |out - ref| <= (e^(2 eps) - 1) * R + 64 * 2^-24 * M

and twice that between the fused kernel and the unfused pair (each within the bound of the reference).
Measured on the MI355X: max err / bound between 0.003 and 0.013 over the cases below (below 0.001 in
the range-guard case, whose large logit widens eps); fused and unfused outputs were bit-identical in
every case but that one, and every case but that one asserts it: the two kernels run the same
functions (csrc/conv1x1_core.h, csrc/softmax9.h), so the same products in the same order.  (The two
kernels' guarded blocks cover different pixels: the range-guard case keeps the 2 * bound.)
"""
import pytest
import torch

from mask_upsample_ref import reference as _reference
from stereoanywhere_amd import _native as N, ops

pytestmark = pytest.mark.gpu
dev = "cuda"

SHAPES = [(1, 1, 1), (2, 7, 13), (1, 5, 16), (1, 3, 17), (2, 9, 33)]


def _case(B, Cin, H, W, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.relu(torch.randn(B, Cin, H, W, generator=g)).to(dev)
    w = (0.05 * torch.randn(144, Cin, 1, 1, generator=g)).to(dev)
    b = torch.randn(144, generator=g).to(dev)
    flow = (5 * torch.randn(B, 1, H, W, generator=g)).to(dev)
    return x, w, b, flow


def _unfused(x, ws, b, scale, flow):
    """sa_conv1x1 + sa_convex_upsample on the same inputs.  sa_conv1x1 takes H*W % 4 == 0 only: it runs
    on the flat plane padded to a multiple of 4 (it is a per-pixel product; the pad columns are cut)."""
    B, Cin, H, W = x.shape
    P = H * W
    xp = torch.zeros((B, Cin, 1, (P + 3) // 4 * 4), device=dev)
    xp[..., :P] = x.reshape(B, Cin, 1, P)
    z = ops.conv1x1(xp, ws, 144, b, scale)[..., :P].reshape(B, 144, H, W).contiguous()
    return ops.convex_upsample(flow, z, 4)


def _check(got, x, w, b, scale, flow, ws, label, bit_equal=True):
    ref, bound = _reference(x, w, b, scale, flow)
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{label}: max err {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    assert torch.isfinite(got).all()
    assert bool((err <= bound).all()), f"{label}: err / bound {ratio}"
    pair = _unfused(x, ws, b, scale, flow)
    d = (got.double() - pair.double()).abs()
    print(f"{label}: max |fused - unfused| {float(d.max()):.3e}, bit-identical {torch.equal(got, pair)}")
    assert bool((d <= 2 * bound).all())
    if bit_equal:
        assert torch.equal(got, pair), f"{label}: fused and unfused outputs differ"


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_mask_upsample_vs_float64(B, H, W, scale):
    """Cin = 256 (the model's): one pixel, ragged tiles (H*W % 4 != 0, W % 16 != 0), more than one
    48-pixel block, two images; every shape's border pixels read the zero padding."""
    x, w, b, flow = _case(B, 256, H, W, 100 * H + W)
    ws = ops.conv1x1_weights(w)
    assert ws is not None
    N.lib().sa_mask_upsample_redo_blocks(1)
    got = ops.mask_upsample(x, ws, b, scale, flow)
    assert got.shape == (B, 1, 4 * H, 4 * W) and got.dtype == torch.float32
    _check(got, x, w, b, scale, flow, ws, f"{B}x256 {H}x{W} scale {scale}")
    assert N.lib().sa_mask_upsample_redo_blocks(1) == 0
    again = ops.mask_upsample(x, ws, b, scale, flow)
    assert torch.equal(got, again)


@pytest.mark.parametrize("Cin", [128, 64])
def test_mask_upsample_other_cin(Cin):
    x, w, b, flow = _case(2, Cin, 7, 13, Cin)
    ws = ops.conv1x1_weights(w)
    N.lib().sa_mask_upsample_redo_blocks(1)
    got = ops.mask_upsample(x, ws, None, 0.25, flow)
    _check(got, x, w, torch.zeros_like(b), 0.25, flow, ws, f"2x{Cin} 7x13 no bias")
    assert N.lib().sa_mask_upsample_redo_blocks(1) == 0


def test_mask_upsample_strided_views_keep_poison():
    """x and out as batch-strided views inside larger buffers: nothing outside the views is read into
    the result or written."""
    B, H, W = 2, 9, 33
    x, w, b, flow = _case(B, 256, H, W, 7)
    ws = ops.conv1x1_weights(w)
    big = torch.full((B, 256 + 48, H, W), float("nan"), device=dev)
    big[:, 16:272] = x
    outb = torch.full((B, 3, 4 * H, 4 * W), 7.0, device=dev)
    N.lib().sa_mask_upsample_redo_blocks(1)
    got = ops.mask_upsample(big[:, 16:272], ws, b, 0.25, flow, out=outb[:, 1:2])
    assert got.data_ptr() == outb[:, 1:2].data_ptr()
    _check(got.contiguous(), x, w, b, 0.25, flow, ws, "strided views")
    assert N.lib().sa_mask_upsample_redo_blocks(1) == 0
    assert torch.all(outb[:, 0] == 7.0) and torch.all(outb[:, 2] == 7.0)
    assert torch.equal(got.contiguous(), ops.mask_upsample(x, ws, b, 0.25, flow))
    assert torch.isnan(big[:, :16]).all() and torch.isnan(big[:, 272:]).all() and torch.equal(big[:, 16:272], x)


def test_mask_upsample_range_guard():
    """One input element beyond the f16 range: its block computes its logits with fp32 FMAs
    (counted); the output is finite and within the bound."""
    B, H, W = 2, 9, 33
    x, w, b, flow = _case(B, 256, H, W, 9)
    x[1, 37, 4, 20] = 7e4
    ws = ops.conv1x1_weights(w)
    N.lib().sa_mask_upsample_redo_blocks(1)
    got = ops.mask_upsample(x, ws, b, 0.25, flow)
    redone = int(N.lib().sa_mask_upsample_redo_blocks(1))
    print("redone blocks", redone)
    assert redone == 1
    _check(got, x, w, b, 0.25, flow, ws, "range guard", bit_equal=False)


def test_mask_upsample_argument_checks():
    x, w, b, flow = _case(1, 256, 4, 8, 3)
    ws = ops.conv1x1_weights(w)
    with pytest.raises(RuntimeError, match="Cin"):
        ops.mask_upsample(x[:, :96].contiguous(), ws, b, 0.25, flow)
    with pytest.raises(RuntimeError, match="flow_x"):
        ops.mask_upsample(x, ws, b, 0.25, flow[:, :, :2].contiguous())
    with pytest.raises(RuntimeError, match="wsplit"):
        ops.mask_upsample(x, ops.conv1x1_weights(w[:64]), b, 0.25, flow)
    # the C entry refuses a Cin it has no kernel for (SA_E_ARG), whatever the wrapper checks
    rc = N.lib().sa_mask_upsample(x.data_ptr(), 96 * 32, 1, 96, 4, 8, ws.data_ptr(), None, 0.25, flow.data_ptr(),
                                  torch.empty(1, 1, 16, 32, device=dev).data_ptr(), 16 * 32, None)
    assert rc != 0

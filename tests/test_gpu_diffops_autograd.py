"""stereoanywhere_amd.diffops on the GPU: the autograd layer over the inference kernels and the HIP
adjoints of csrc/diffops_backward.hip.  Forward bits, a chain through torch layers against the torch
formulation (the 4 e_ref rule of tests/test_gpu_diffops_backward.py, measured on the parameters'
gradients), what the functions save for backward, grad mode, autocast and the refusals."""
import copy

import numpy as np
import pytest
import torch

import diffops_ref as ref
from stereoanywhere_amd import diffops, ops

pytestmark = pytest.mark.gpu
dev = "cuda"


def _volumes(W1, W2, seed=0, B=2, H=3):
    gen = torch.Generator().manual_seed(seed)
    return [(4.0 * torch.randn((B, 1, H, W1, W2), generator=gen)).to(dev) for _ in range(2)]


# ------------------------------------------------------------------------------ forward bits
@pytest.mark.parametrize("W", [44, 300])
def test_softargmin_forward_bits(W):
    vd, vc = _volumes(W, W)
    B, _, H, _, _ = vd.shape
    od, oc = ops.softargmin_conf(vd, vc, (vd.stride(0), vd.stride(2), vd.stride(3), vd.stride(4)), (B, H, W, W))
    want = (od[:, 0:1], od[:, 1:2], oc[:, 0:1], oc[:, 1:2])
    plain = diffops.softargmin_conf(vd, vc)
    with_grad = diffops.softargmin_conf(vd.clone().requires_grad_(), vc.clone().requires_grad_())
    singles = (diffops.estimate_left_disparity(vd), diffops.estimate_right_disparity(vd),
               diffops.estimate_left_confidence(vc), diffops.estimate_right_confidence(vc))
    for w, a, b, s in zip(want, plain, with_grad, singles):
        assert a.shape == (B, 1, H, W) and a.grad_fn is None and b.grad_fn is not None
        assert torch.equal(a, w) and torch.equal(b, w) and torch.equal(s, w)
    # vol_pad is a slice of the output
    assert torch.equal(diffops.estimate_left_disparity(vd, vol_pad=[3, 5]), want[0][..., 3:W - 5])
    assert torch.equal(diffops.estimate_right_disparity(vd, [2, 0]), want[1][..., 2:])
    # one volume only
    assert diffops.softargmin_conf(None, vc)[:2] == (None, None)
    assert torch.equal(diffops.softargmin_conf(vd, None)[1], want[1])


def test_softargmin_forward_unequal_widths():
    vd, vc = _volumes(37, 50)
    got = diffops.softargmin_conf(vd, vc)
    # the plug-in's forward is ops.softargmin_conf_maps, with and without a graph: the same bits
    strides = (vd.stride(0), vd.stride(2), vd.stride(3), vd.stride(4))
    raw = ops.softargmin_conf_maps(vd, vc, strides, (2, 3, 37, 50))
    with_grad = diffops.softargmin_conf(vd.clone().requires_grad_(), vc.clone().requires_grad_())
    for a, b, r in zip(got, with_grad, raw):
        assert torch.equal(a, r) and torch.equal(b, r) and b.grad_fn is not None
    want = (ref.left_disparity(vd[:, 0].double().cpu()), ref.right_disparity(vd[:, 0].double().cpu()),
            ref.left_confidence(vc[:, 0].double().cpu()), ref.right_confidence(vc[:, 0].double().cpu()))
    for a, w, tol in zip(got, want, (2e-4, 2e-4, 4e-6, 4e-6)):   # ~2^-18 of the maps' ranges (50, 1)
        assert a.shape == (2, 1) + tuple(w.shape[1:])
        assert (a[:, 0].double().cpu() - w).abs().max() <= tol


@pytest.mark.parametrize("use_scale", [True, False])
def test_convex_upflow_forward_bits(use_scale):
    gen = torch.Generator().manual_seed(3)
    flow = (10.0 * torch.randn((2, 1, 5, 7), generator=gen)).to(dev)
    mask = torch.randn((2, 144, 5, 7), generator=gen).to(dev)
    want = ops.convex_upsample(flow, mask, 4)
    if not use_scale:   # the factor is a power of two: dividing by it is exact
        want = want / 4
    a = diffops.convex_upflow(flow, mask, use_scale_factor=use_scale)
    b = diffops.convex_upflow(flow.clone().requires_grad_(), mask, use_scale_factor=use_scale)
    assert a.grad_fn is None and b.grad_fn is not None
    assert torch.equal(a, want) and torch.equal(b, want)
    # a non-contiguous mask is made contiguous
    wide = torch.zeros((2, 150, 5, 7), device=dev)
    wide[:, 3:147] = mask
    assert torch.equal(diffops.convex_upflow(flow, wide[:, 3:147].transpose(2, 3).contiguous().transpose(2, 3),
                                             use_scale_factor=use_scale), want)


# ------------------------------------------------------------------------------------- chain
class _Chain(torch.nn.Module):
    """Two small 3-D convs make the volumes; flow and mask are parameters."""

    def __init__(self, W, h, w):
        super().__init__()
        gen = torch.Generator().manual_seed(5)
        self.conv_d = torch.nn.Conv3d(2, 1, 3, padding=1)
        self.conv_c = torch.nn.Conv3d(2, 1, 3, padding=1)
        for p in list(self.conv_d.parameters()) + list(self.conv_c.parameters()):
            p.data = torch.randn(p.shape, generator=gen)
        self.flow = torch.nn.Parameter(10.0 * torch.randn((2, 1, h, w), generator=gen))
        self.mask = torch.nn.Parameter(4.0 * torch.randn((2, 144, h, w), generator=gen))
        self.x = torch.nn.Parameter(torch.randn((2, 2, 3, W, W), generator=gen), requires_grad=False)
        self.wts = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.randn((2, 1, 3, W), generator=gen), requires_grad=False) for _ in range(4)] +
            [torch.nn.Parameter(torch.randn((2, 1, 4 * h, 4 * w), generator=gen), requires_grad=False)])

    def loss(self, how):
        vd, vc = self.conv_d(self.x), self.conv_c(self.x)
        if how == "torch":
            maps = (ref.left_disparity(vd[:, 0]), ref.right_disparity(vd[:, 0]), ref.left_confidence(vc[:, 0]),
                    ref.right_confidence(vc[:, 0]))
            maps = [m[:, None] for m in maps]
            up = ref.convex_upflow(self.flow, 0.25 * self.mask, 4)
        else:
            if how == "joint":
                maps = diffops.softargmin_conf(vd, vc)
            else:
                maps = (diffops.estimate_left_disparity(vd), diffops.estimate_right_disparity(vd),
                        diffops.estimate_left_confidence(vc), diffops.estimate_right_confidence(vc))
            up = diffops.convex_upflow(self.flow, 0.25 * self.mask)
        return sum((m * w).sum() for m, w in zip(list(maps) + [up], self.wts))

    def grads(self, how):
        self.zero_grad()
        self.loss(how).backward()
        return {n: p.grad.detach().double().cpu().numpy() for n, p in self.named_parameters() if p.grad is not None}


def test_chain_matches_torch_formulation():
    base = _Chain(24, 5, 7)
    want64 = copy.deepcopy(base).double().grads("torch")
    want32 = copy.deepcopy(base).grads("torch")
    model = copy.deepcopy(base).to(dev)
    assert set(want64) == {"conv_d.weight", "conv_d.bias", "conv_c.weight", "conv_c.bias", "flow", "mask"}
    for how in ("joint", "separate"):
        got = model.grads(how)
        assert set(got) == set(want64)
        for name in sorted(want64):
            e_ref = np.abs(want32[name] - want64[name]).max()
            err = np.abs(got[name] - want64[name]).max()
            print(f"{how} {name}: err {err:.3g}, e_ref {e_ref:.3g}, err/e_ref {err / max(e_ref, 1e-300):.3g}")
            assert err <= 4 * e_ref, (how, name)


# ------------------------------------------------------------------------------ saved memory
def _saved_bytes(fn):
    seen = {}

    def pack(t):
        seen[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = fn()
    return out, sum(seen.values())


def test_saved_memory():
    B, H, W1, W2 = 2, 3, 37, 50
    vd, vc = (v.requires_grad_() for v in _volumes(W1, W2))
    outs, nbytes = _saved_bytes(lambda: diffops.softargmin_conf(vd, vc))
    vol_bytes = 2 * 4 * B * H * W1 * W2
    print(f"soft-argmin: saved {nbytes} bytes, volumes {vol_bytes}")
    assert 0 < nbytes <= vol_bytes + 16 * B * H * (W1 + W2)
    sum(o.sum() for o in outs).backward()
    assert vd.grad is not None and vc.grad is not None
    flow = torch.randn((2, 1, 5, 7), device=dev, requires_grad=True)
    mask = torch.randn((2, 144, 5, 7), device=dev, requires_grad=True)
    up, nbytes = _saved_bytes(lambda: diffops.convex_upflow(flow, mask))
    print(f"up-sampling: saved {nbytes} bytes, flow + mask {4 * (flow.numel() + mask.numel())}")
    assert 0 < nbytes <= 4 * (flow.numel() + mask.numel())
    up.sum().backward()
    assert flow.grad is not None and mask.grad is not None


# --------------------------------------------------------------------- grad mode and dtypes
def test_grad_mode():
    vd, vc = (v.requires_grad_() for v in _volumes(44, 44))
    flow = torch.randn((2, 1, 5, 7), device=dev, requires_grad=True)
    mask = torch.randn((2, 144, 5, 7), device=dev)
    with torch.no_grad():
        assert all(o.grad_fn is None for o in diffops.softargmin_conf(vd, vc))
        assert diffops.convex_upflow(flow, mask).grad_fn is None
    assert all(o.grad_fn is None for o in diffops.softargmin_conf(vd.detach(), vc.detach()))
    assert diffops.convex_upflow(flow.detach(), mask).grad_fn is None
    # only the inputs that ask get a gradient; an unused output's gradient is not materialised
    dL = diffops.softargmin_conf(vd, vc.detach())[0]
    dL.sum().backward()
    assert vd.grad is not None and vc.grad is None and torch.isfinite(vd.grad).all()
    diffops.convex_upflow(flow, mask).sum().backward()
    assert flow.grad is not None and mask.grad is None
    # double backward is not built (the weights require grad, so the first backward's result is in the graph)
    vd.grad = None
    cL = diffops.estimate_left_confidence(vd)
    gv, = torch.autograd.grad((cL * torch.ones_like(cL, requires_grad=True)).sum(), vd, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gv.sum().backward()
    up = diffops.convex_upflow(flow, mask)
    gf, = torch.autograd.grad((up * torch.ones_like(up, requires_grad=True)).sum(), flow, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gf.sum().backward()


def test_autocast_fp16_volume():
    v16 = _volumes(44, 44)[0].half().requires_grad_()
    with torch.autocast("cuda"):
        dL, dR, cL, cR = diffops.softargmin_conf(v16, v16)
        up = diffops.convex_upflow(torch.randn((2, 1, 5, 7), device=dev).half(),
                                   torch.randn((2, 144, 5, 7), device=dev).half())
    assert all(o.dtype == torch.float32 for o in (dL, dR, cL, cR, up))
    (dL.sum() + cR.sum()).backward()
    assert v16.grad.dtype == torch.float16 and torch.isfinite(v16.grad).all() and v16.grad.abs().max() > 0


def test_refusals():
    vd = _volumes(8, 8)[0]
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        diffops.softargmin_conf(vd.cpu(), None)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        diffops.estimate_right_confidence(vd.cpu())
    with pytest.raises(RuntimeError, match=r"\[B,1,H,W1,W2\]"):
        diffops.estimate_left_disparity(vd[:, 0])
    flow = torch.randn((2, 1, 5, 7), device=dev)
    mask = torch.randn((2, 144, 5, 7), device=dev)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        diffops.convex_upflow(flow.cpu(), mask.cpu())
    with pytest.raises(RuntimeError, match="D == 1"):
        diffops.convex_upflow(torch.cat([flow, flow], 1), mask)
    with pytest.raises(RuntimeError, match="n_downsample must be 0..3"):
        diffops.convex_upflow(flow, mask, n_downsample=4)
    with pytest.raises(RuntimeError, match="mask must be"):
        diffops.convex_upflow(flow, mask[:, :36])

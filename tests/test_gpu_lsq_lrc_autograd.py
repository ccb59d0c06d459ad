"""stereoanywhere_amd.diffops.softlrc / softlrc_conf / weighted_lsq on the GPU: the autograd layer over
the inference kernels and the HIP adjoints of csrc/lsq_backward.hip.  Forward bits, a chain as the
reference's forward runs it against the torch formulation (the 4 e_ref rule of
tests/test_gpu_lsq_lrc_backward.py, measured on the parameters' gradients), what the functions save for
backward, grad mode, fp16 inputs and the refusals."""
import copy

import numpy as np
import pytest
import torch

import lsq_lrc_ref as ref
from stereoanywhere_amd import diffops, ops

pytestmark = pytest.mark.gpu
dev = "cuda"
B, H, W = 2, 9, 33


def _maps(conf=True):
    d2, d3 = (torch.from_numpy(a).to(dev) for a in ref.lrc_inputs(B, H, W, 6.0, seed=9))
    gen = torch.Generator().manual_seed(4)
    c2, c3 = (torch.rand((B, 1, H, W), generator=gen).to(dev) for _ in range(2))
    mde = (3.0 * torch.randn((B, 2, H, W), generator=gen)).to(dev)
    return d2, d3, c2, c3, mde


# ------------------------------------------------------------------------------ forward bits
def test_forward_bits_and_grad_fn():
    d2, d3, c2, c3, mde = _maps()
    want = ops.softlrc(d2, d3)
    wantc = ops.softlrc(d2, d3, c2, c3, 1.0)
    joint = ops.softlrc_joint(torch.cat([d2, d3], 1), torch.cat([c2, c3], 1), 1.0)
    assert torch.equal(wantc[0], joint[:, :1]) and torch.equal(wantc[1], joint[:, 1:])
    disp, confx = torch.cat([d2, d3], 1), joint
    sc, sh = ops.weighted_lsq(mde.reshape(B, -1), disp.reshape(B, -1), confx.reshape(B, -1))
    for grad in (False, True):
        r = (lambda t: t.clone().requires_grad_()) if grad else (lambda t: t)
        with torch.no_grad():
            outs = (diffops.softlrc(r(d2), r(d3)), diffops.softlrc_conf(r(d2), r(d3), r(c2), r(c3)),
                    diffops.weighted_lsq(r(mde), r(disp), r(confx)))
        assert all(o.grad_fn is None for pair in outs for o in pair)
        assert torch.equal(outs[0][0], want[0]) and torch.equal(outs[0][1], want[1])
        assert torch.equal(outs[1][0], wantc[0]) and torch.equal(outs[1][1], wantc[1])
        assert outs[2][0].shape == (B, 1, 1, 1) and outs[2][1].shape == (B, 1, 1, 1)
        assert torch.equal(outs[2][0].flatten(), sc) and torch.equal(outs[2][1].flatten(), sh)
    # inputs that do not require grad: the plain calls with grad mode on, too
    assert all(o.grad_fn is None for o in diffops.softlrc_conf(d2, d3, c2, c3) + diffops.weighted_lsq(mde, disp, confx))
    # with a graph: the same bits
    s2, s3 = diffops.softlrc(d2.clone().requires_grad_(), d3)
    t2, t3 = diffops.softlrc_conf(d2, d3, c2.clone().requires_grad_(), c3)
    a, b = diffops.weighted_lsq(mde, disp.clone().requires_grad_(), confx)
    assert all(o.grad_fn is not None for o in (s2, s3, t2, t3, a, b))
    assert torch.equal(s2, want[0]) and torch.equal(s3, want[1]) and torch.equal(t2, wantc[0]) and torch.equal(t3, wantc[1])
    assert torch.equal(a.flatten(), sc) and torch.equal(b.flatten(), sh)
    # any [B, ...] maps, flattened per sample
    a2, b2 = diffops.weighted_lsq(mde.reshape(B, 2 * H, W), disp.reshape(B, 2 * H, W), confx.reshape(B, 2 * H, W))
    assert torch.equal(a2, a) and torch.equal(b2, b)
    # the scale and shift against the float64 restatement: fp32 products in the sums (1e-5 of the values)
    rs, rt = ref.weighted_lsq(*(t.reshape(B, -1).cpu() for t in (mde, disp, confx)), torch.float64)
    assert (sc.double().cpu() - rs).abs().max() <= 1e-5 * max(1.0, float(rs.abs().max()))
    assert (sh.double().cpu() - rt).abs().max() <= 1e-5 * max(1.0, float(rt.abs().max()))


# ------------------------------------------------------------------------------------- chain
class _Chain(torch.nn.Module):
    """As the reference's forward: a small conv makes the two disparity maps and (through a sigmoid) the
    two confidences; softlrc, the product with the confidences, weighted_lsq against a fixed mono map,
    the scaled mono map and an L1 loss."""

    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(5)
        self.conv = torch.nn.Conv2d(3, 4, 3, padding=1)
        for p in self.conv.parameters():
            p.data = 0.6 * torch.randn(p.shape, generator=gen)
        self.x = torch.nn.Parameter(torch.randn((B, 3, H, W), generator=gen), requires_grad=False)
        self.mde = torch.nn.Parameter(3.0 * torch.rand((B, 2, H, W), generator=gen) + 0.2, requires_grad=False)
        self.target = torch.nn.Parameter(4.0 * torch.randn((B, 2, H, W), generator=gen), requires_grad=False)

    def loss(self, how):
        y = self.conv(self.x)
        d2, d3 = y[:, 0:1] + 1.0, y[:, 1:2] + 1.0
        c2, c3 = torch.sigmoid(y[:, 2:3]), torch.sigmoid(y[:, 3:4])
        disp = torch.cat([d2, d3], 1)
        if how == "torch":
            s2, s3 = ref.softlrc(d2, d3)
            confx = torch.cat([c2 * s2, c3 * s3], 1)
            scale, shift = ref.weighted_lsq(self.mde.reshape(B, -1), disp.reshape(B, -1), confx.reshape(B, -1), y.dtype)
            scale, shift = scale.reshape(B, 1, 1, 1), shift.reshape(B, 1, 1, 1)
        else:
            if how == "fused":
                s2, s3 = diffops.softlrc_conf(d2, d3, c2, c3)
                confx = torch.cat([s2, s3], 1)
            else:
                s2, s3 = diffops.softlrc(d2, d3)
                confx = torch.cat([c2 * s2, c3 * s3], 1)
            scale, shift = diffops.weighted_lsq(self.mde, disp, confx)
        return (scale * self.mde + shift - self.target).abs().mean()

    def grads(self, how):
        self.zero_grad()
        self.loss(how).backward()
        return {n: p.grad.detach().double().cpu().numpy() for n, p in self.named_parameters() if p.grad is not None}


def test_chain_matches_torch_formulation():
    base = _Chain()
    want64 = copy.deepcopy(base).double().grads("torch")
    want32 = copy.deepcopy(base).grads("torch")
    model = copy.deepcopy(base).to(dev)
    assert set(want64) == {"conv.weight", "conv.bias"}
    for how in ("separate", "fused"):
        got = model.grads(how)
        assert set(got) == set(want64)
        for name in sorted(want64):
            e_ref = np.abs(want32[name] - want64[name]).max()
            err = np.abs(got[name] - want64[name]).max()
            print(f"{how} {name}: err {err:.3g}, e_ref {e_ref:.3g} ({e_ref / np.abs(want64[name]).max():.2g} of max|g|), "
                  f"err/e_ref {err / max(e_ref, 1e-300):.3g}")
            assert np.abs(want64[name]).max() > 0
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
    d2, d3, c2, c3, mde = (t.requires_grad_() for t in _maps())
    outs, nbytes = _saved_bytes(lambda: diffops.softlrc_conf(d2, d3, c2, c3))
    print(f"softlrc_conf: saved {nbytes} bytes, the four maps {4 * 4 * B * H * W}")
    assert 0 < nbytes <= 4 * 4 * B * H * W
    sum(o.sum() for o in outs).backward()
    assert all(t.grad is not None for t in (d2, d3, c2, c3))
    disp, confx = torch.cat([d2, d3], 1).detach().requires_grad_(), torch.cat(outs, 1).detach().requires_grad_()
    (scale, shift), nbytes = _saved_bytes(lambda: diffops.weighted_lsq(mde, disp, confx))
    maps = 3 * 4 * B * 2 * H * W
    print(f"weighted_lsq: saved {nbytes} bytes, the three maps {maps}")
    assert 0 < nbytes <= maps + B * (2 * 4 + 8 * ops.LSQ_REC)   # + scale, shift and the record
    (scale.sum() + shift.sum()).backward()
    assert all(t.grad is not None for t in (mde, disp, confx))


# --------------------------------------------------------------------- grad mode and dtypes
def test_grad_mode():
    d2, d3, c2, c3, mde = _maps()
    d2 = d2.requires_grad_()
    # only the inputs that ask get a gradient; an unused output's gradient is not materialised
    s2, s3 = diffops.softlrc_conf(d2, d3, c2, c3)
    s3.sum().backward()
    assert d2.grad is not None and torch.isfinite(d2.grad).all() and d2.grad.abs().max() > 0 and c2.grad is None
    want = ops.softlrc_backward(d2.detach(), d3, c2, c3, 1.0, None, torch.ones_like(d3), True, False)[0]
    assert torch.equal(d2.grad, want)
    disp = torch.cat([d2.detach(), d3], 1)
    confx = torch.cat([s2, s3], 1).detach().requires_grad_()
    scale, shift = diffops.weighted_lsq(mde, disp, confx)
    shift.sum().backward()
    assert confx.grad is not None and confx.grad.abs().max() > 0
    sc, sh, rec = ops.weighted_lsq_stats(mde.reshape(B, -1), disp.reshape(B, -1), confx.detach().reshape(B, -1))
    want = ops.weighted_lsq_backward(mde.reshape(B, -1), disp.reshape(B, -1), confx.detach().reshape(B, -1), sc, sh, rec,
                                     None, torch.ones(B, device=dev), False, False, True)[2]
    assert torch.equal(confx.grad.reshape(B, -1), want)
    # double backward is not built
    d2.grad = None
    s2, _ = diffops.softlrc(d2, d3)
    gd, = torch.autograd.grad((s2 * torch.ones_like(s2, requires_grad=True)).sum(), d2, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gd.sum().backward()


def test_fp16_inputs():
    d2, d3, c2, c3, mde = _maps()
    h2, h3 = d2.half().requires_grad_(), d3.half().requires_grad_()
    s2, s3 = diffops.softlrc(h2, h3)
    assert s2.dtype == torch.float32 and s3.dtype == torch.float32
    assert torch.equal(s2, ops.softlrc(h2.detach().float(), h3.detach().float())[0])
    (s2.sum() + s3.sum()).backward()
    for t in (h2, h3):
        assert t.grad.dtype == torch.float16 and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0
    m16 = mde.half().requires_grad_()
    disp = torch.cat([d2, d3], 1).half().requires_grad_()
    confx = torch.cat([c2, c3], 1)
    scale, shift = diffops.weighted_lsq(m16, disp, confx)
    assert scale.dtype == torch.float16 and scale.shape == (B, 1, 1, 1)   # the caller's mde dtype
    (scale.float().sum() + shift.float().sum()).backward()
    for t in (m16, disp):
        assert t.grad.dtype == torch.float16 and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0


def test_refusals():
    d2, d3, c2, c3, mde = _maps()
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        diffops.softlrc(d2.cpu(), d3.cpu())
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        diffops.softlrc_conf(d2, d3, c2.cpu(), c3)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        diffops.weighted_lsq(mde.cpu(), mde.cpu(), mde.cpu())
    with pytest.raises(RuntimeError, match=r"disp2 must be \[B,1,H,W\]"):
        diffops.softlrc(mde, mde)
    with pytest.raises(RuntimeError, match="disp3 must have the shape of disp2"):
        diffops.softlrc(d2, d3[:, :, :, 1:])
    with pytest.raises(RuntimeError, match="conf2 and conf3 must be given"):
        diffops.softlrc_conf(d2, d3, None, c3)
    with pytest.raises(RuntimeError, match="conf must be"):
        diffops.weighted_lsq(mde, mde, mde[:, :1])
    with pytest.raises(RuntimeError, match="floating-point"):
        diffops.weighted_lsq(mde, mde, mde.long())

"""Autograd behaviour of stereoanywhere_amd.diffops.truncate_volume / volume_stage on the GPU: the
gradient is the upstream gradient times the recomputed factor, only the two maps are saved, corrupted
outputs are detached, and the stage composes with the differentiable correlation plug-in."""
import numpy as np
import pytest
import torch

import volume_stage_ref as R
from stereoanywhere_amd import diffops
from stereoanywhere_amd.corr import HipCorrBlock1D
from stereoanywhere_amd.diffops import VolumeCorruption

pytestmark = pytest.mark.gpu
dev = "cuda"
SHAPE = (2, 3, 37, 37)


def inputs():
    c = R.random_case(7, *SHAPE)
    return c, {k: v.to(dev) for k, v in c.items()}


@pytest.mark.parametrize("atten", [0.9, 0.1])
def test_gradient_is_upstream_times_factor(atten):
    c, t = inputs()
    vol = t["volume"].clone().requires_grad_()
    out = diffops.truncate_volume(vol, t["disp"], t["conf"], atten)
    assert out.requires_grad and out.grad_fn is not None
    R.assert_close(out, R.stage(c["volume"], trunc=(c["disp"], c["conf"], atten), dtype=torch.float64), "forward")
    g = torch.randn(SHAPE[0], 1, *SHAPE[1:], generator=torch.Generator().manual_seed(3))
    out.backward(g.to(dev))
    torch.cuda.synchronize()
    f64 = R.trunc_factor(c["disp"], c["conf"], atten, SHAPE[3], torch.float64)
    R.assert_close(vol.grad, g.double() * f64, "grad_volume")


def test_saves_two_maps_and_nothing_volume_sized():
    _, t = inputs()
    vol = t["volume"].clone().requires_grad_()
    out = diffops.truncate_volume(vol, t["disp"], t["conf"], 0.9)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 2
    assert [tuple(s.shape) for s in saved] == [tuple(t["disp"].shape)] * 2
    assert all(s.numel() * SHAPE[3] == vol.numel() for s in saved)
    assert saved[0].data_ptr() == t["disp"].data_ptr() and saved[1].data_ptr() == t["conf"].data_ptr()


def test_maps_get_no_gradient_and_plain_call_without_grad():
    _, t = inputs()
    vol = t["volume"].clone().requires_grad_()
    disp, conf = t["disp"].clone().requires_grad_(), t["conf"].clone().requires_grad_()
    out = diffops.truncate_volume(vol, disp, conf, 0.9)
    out.sum().backward()
    assert vol.grad is not None and disp.grad is None and conf.grad is None
    # nothing that requires grad among the differentiable inputs, or no_grad: the plain call
    plain = diffops.truncate_volume(t["volume"], disp, conf, 0.9)
    assert plain.grad_fn is None and not plain.requires_grad
    with torch.no_grad():
        quiet = diffops.truncate_volume(vol, t["disp"], t["conf"], 0.9)
    assert quiet.grad_fn is None and torch.equal(quiet, plain) and torch.equal(quiet, out.detach())


def test_double_backward_raises():
    _, t = inputs()
    vol = t["volume"].clone().requires_grad_()
    out = diffops.truncate_volume(vol, t["disp"], t["conf"], 0.9)
    # the weights require grad, so the first backward's result is in the graph
    g, = torch.autograd.grad((out * torch.ones_like(out, requires_grad=True)).sum(), vol, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_corrupted_outputs_are_detached_and_uncorrupted_backpropagate():
    _, t = inputs()
    trunc = (t["disp"], t["conf"], 0.9)
    for kind in ("roll", "noise", "zero"):
        vol, mono = t["volume"].clone().requires_grad_(), t["volume"].clone().requires_grad_()
        plan = VolumeCorruption("stereo", kind, 1, 5 if kind == "roll" else 0)
        s, m = diffops.volume_stage(vol, mono, t["mde"], plan, trunc, t["noise"])
        assert not s.requires_grad and s.grad_fn is None and m is mono
        plan = VolumeCorruption("mono", kind, 1, 5 if kind == "roll" else 0)
        s, m = diffops.volume_stage(vol, mono, t["mde"], plan, trunc, t["noise"])
        assert not m.requires_grad and m.grad_fn is None
        assert s.requires_grad and s.grad_fn is not None      # the stereo volume is only truncated
        s.sum().backward()
        assert vol.grad is not None and mono.grad is None
    vol = t["volume"].clone().requires_grad_()
    s, m = diffops.volume_stage(vol, t["volume"], None, None, trunc)
    assert m is t["volume"] and s.grad_fn is not None
    s.sum().backward()
    torch.cuda.synchronize()
    R.assert_close(vol.grad, R.trunc_factor(*[x.cpu() for x in trunc[:2]], 0.9, SHAPE[3], torch.float64), "grad of the sum")


def _chain(f2, f3, stage, coords, Rw, L, Rad):
    f2, f3 = f2.clone().requires_grad_(), f3.clone().requires_grad_()
    vol = HipCorrBlock1D.corr(f2, f3)                       # [B,H,W1,1,W2]
    B, H, W1, _, W2 = vol.shape
    v5 = stage(vol.squeeze(3).unsqueeze(1))                  # [B,1,H,W1,W2]
    blk = HipCorrBlock1D(v5.squeeze(1).unsqueeze(3), num_levels=L, radius=Rad)
    (blk(coords) * Rw).sum().backward()
    torch.cuda.synchronize()
    return f2.grad.cpu().numpy().astype(np.float64), f3.grad.cpu().numpy().astype(np.float64)


def test_backpropagates_through_the_correlation_block():
    """HipCorrBlock1D(volume_stage(...)[0]) -> fmap2 / fmap3 through corr, against the same chain with
    the stage written in torch ops (T * vol, T from torch.sigmoid on the GPU), within the bound
    tests/test_gpu_corr_backward.py::test_gradients_through_the_contract uses for this path:
    |err| <= (K + L + 8) 2^-24 mag, K = W2 for f2.grad and W1 for f3.grad, mag = the chain on absolute
    values (the lookup's coefficients are non-negative, so that is the sum of the absolute terms)."""
    B, C, H, W, L, Rad = 2, 40, 3, 37, 4, 4
    rng = np.random.default_rng(5)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    f2, f3 = g(rng.standard_normal((B, C, H, W))), g(rng.standard_normal((B, C, H, W)))
    Rw = g(rng.standard_normal((B, L * (2 * Rad + 1), H, W)))
    coords = g(np.concatenate([rng.random((B, 1, H, W)) * (W + 6) - 3, np.zeros((B, 1, H, W))], 1))
    c = R.random_case(9, B, H, W, W)
    disp, conf = c["disp"].to(dev), c["conf"].to(dev)
    atten = 0.9

    def hip_stage(v):
        out = diffops.volume_stage(v, v.detach(), None, None, (disp, conf, atten))[0]
        assert out.grad_fn is not None
        return out

    def torch_stage(v):
        j = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, 1, W, 1)
        k = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, 1, 1, W)
        t = conf.unsqueeze(4)
        T = 1 * (1 - t) + t * (torch.sigmoid((j - disp.unsqueeze(4)) - k) * (1 - atten) + atten)
        return T.detach() * v

    got = _chain(f2, f3, hip_stage, coords, Rw, L, Rad)
    want = _chain(f2, f3, torch_stage, coords, Rw, L, Rad)
    mag = _chain(f2.abs(), f3.abs(), torch_stage, coords, Rw.abs(), L, Rad)
    U = 2.0 ** -24
    for name, a, b, m in zip(("fmap2.grad", "fmap3.grad"), got, want, mag):
        err, bound = np.abs(a - b), (W + L + 8) * U * m
        ok = bound > 0
        print(f"{name}: max err {err.max():.3g}, max err/bound {(err[ok] / bound[ok]).max():.3g}")
        assert np.abs(b).max() > 0 and np.all(err <= bound)

"""diffops.conv3d_k3 (csrc/conv3d_mfma.hip forward and data gradient, csrc/conv3d_backward.hip weight gradient and
per-sample scale) against the float64 reference of tests/conv3d_k3_ref.py.

Forward and dx are the inference kernel's products and take test_conv3d_mf_vs_float64's criterion: max error over
max |ref| below 2e-6 and below 8 x max(e_fp32, 1e-7), e_fp32 the direct fp32 kernel sa_conv3d on the same inputs.
dw is held elementwise to (R + c) u sum |x| |g|.  Scale equivariance, mixed batches, subsets of
needs_input_grad and the saved tensors are compared on bits."""
import pytest
import torch

import conv3d_k3_ref as R
from invariance_util import same_bits
from stereoanywhere_amd import _native as N, diffops, ops

pytestmark = pytest.mark.gpu
dev = "cuda"


def _run(x, weight, g, x_bounded=True, need=(True, True)):
    """(out, dx, dw) of one conv3d_k3 call under autograd on the GPU; None where not asked for."""
    x = x.to(dev).requires_grad_(need[0])
    weight = weight.to(dev).requires_grad_(need[1])
    out = diffops.conv3d_k3(x, weight, x_bounded=x_bounded)
    out.backward(g.to(dev))
    return out.detach(), x.grad, weight.grad


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def _direct(x, w_t):
    """The direct fp32 kernel on x itself (identity transform)."""
    return ops.conv3d(ops.VolAct(x.to(dev)), w_t.to(dev), w_t.shape[2], stats=False).raw


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("x_bounded", [True, False], ids=["bounded", "scaled"])
def test_against_float64(shape, x_bounded):
    c = R.case(*shape)
    N.lib().sa_conv3d_mf_set_planes(R.PLANES.get(shape, 0))
    try:
        out, dx, dw = _run(c["x"], c["weight"], c["g"], x_bounded)
    finally:
        N.lib().sa_conv3d_mf_set_planes(0)
    for name, got, ref, inp, w in (("out", out, c["out"], c["x"], c["weight"]),
                                   ("dx", dx, c["dx"], c["g"], R.flipped(c["weight"]))):
        e_mf, e_fp32 = _rel(got, ref), _rel(_direct(inp, R.to_taps(w)), ref)
        print(f"{name} {shape}: e_mf {e_mf:.3g}, e_fp32 {e_fp32:.3g}")
        assert e_mf < 2e-6 and e_mf < 8 * max(e_fp32, 1e-7), (name, e_mf, e_fp32)
    err, bound = (dw.double().cpu() - c["dw"]).abs(), R.dw_bound(c["mag"])
    used = (err / bound)[bound > 0]   # (a tap that only ever meets the padding has a zero sum and a zero bound)
    print(f"dw {shape}: at most {float(used.max()):.3g} of the bound is used")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[5]], ids=["8", "32"])
def test_scale_equivariance(shape):
    """A gradient far outside the f16 range gives the unscaled call's bits times its power of two."""
    c = R.case(*shape)
    out, dx, dw = _run(c["x"], c["weight"], c["g"])
    for p in (-40, 30):
        _, dx_p, dw_p = _run(c["x"], c["weight"], c["g"] * 2.0 ** p)
        assert same_bits(dx_p, dx * 2.0 ** p) and same_bits(dw_p, dw * 2.0 ** p), p
    out_s, dx_s, dw_s = _run(c["x"] * 2.0 ** 20, c["weight"], c["g"], x_bounded=False)
    out_1, dx_1, dw_1 = _run(c["x"], c["weight"], c["g"], x_bounded=False)
    assert same_bits(out_s, out_1 * 2.0 ** 20) and same_bits(dw_s, dw_1 * 2.0 ** 20) and same_bits(dx_s, dx_1)
    assert same_bits(dx_1, dx)   # dx does not read x


def test_sample_scale_follows_the_rule():
    t = torch.randn(6, 3, 5, 7, 9, device=dev)
    t[0] *= 2.0 ** -50
    t[1] *= 2.0 ** 40
    t[2] = 0.0
    t[3, 1, 2, 3, 4] = float("inf")
    t[4, 0, 0, 0, 0] = float("nan")
    scale, inv = ops.sample_scale(t, 4)
    want = torch.from_numpy(R.sample_scales(t))
    assert torch.equal(scale.cpu().view(6, 4), want[:, None].expand(6, 4))
    assert torch.equal(inv.cpu(), 1.0 / want)
    amax = (t[[0, 1, 5]].abs().amax(dim=(1, 2, 3, 4)).cpu() * want[[0, 1, 5]])
    assert bool(((amax >= 2.0 ** 13) & (amax < 2.0 ** 14)).all())


def test_mixed_batches():
    """Samples 2^30 apart keep their own bits; an all-zero g gives zeros; a NaN stays in its sample's dx and
    reaches dw."""
    C, B, D, H, W = R.SHAPES[2]
    c = R.case(C, B, D, H, W)
    g = c["g"].clone()
    g[1] *= 2.0 ** 30
    _, dx, dw = _run(c["x"], c["weight"], g)
    for b in range(B):
        _, dx_b, _ = _run(c["x"][b:b + 1], c["weight"], g[b:b + 1])
        assert same_bits(dx[b:b + 1], dx_b), b
    _, dx0, dw0 = _run(c["x"], c["weight"], torch.zeros_like(g))
    assert not bool(dx0.any()) and not bool(dw0.any())
    g = c["g"].clone()
    g[1, 3, 2, 1, 5] = float("nan")
    _, dxn, dwn = _run(c["x"], c["weight"], g)
    _, dx_clean, _ = _run(c["x"][:1], c["weight"], g[:1])
    assert same_bits(dxn[:1], dx_clean) and bool(dxn[1].isnan().any()) and bool(dwn.isnan().any())


def test_subsets_and_saved_tensors():
    c = R.case(*R.SHAPES[4])
    _, dx, dw = _run(c["x"], c["weight"], c["g"])
    _, dx_only, none_w = _run(c["x"], c["weight"], c["g"], need=(True, False))
    _, none_x, dw_only = _run(c["x"], c["weight"], c["g"], need=(False, True))
    assert none_w is None and none_x is None and same_bits(dx_only, dx) and same_bits(dw_only, dw)
    saved = []
    x, w = c["x"].to(dev).requires_grad_(True), c["weight"].to(dev).requires_grad_(True)
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        out = diffops.conv3d_k3(x, w, x_bounded=True)
    assert len(saved) == 2 and {t.data_ptr() for t in saved} == {x.data_ptr(), w.data_ptr()}
    assert out.grad_fn is not None
    with torch.no_grad():
        assert same_bits(diffops.conv3d_k3(x, w, x_bounded=True), out)


def test_refusals_and_the_weight_check():
    x = torch.randn(1, 8, 3, 4, 5, device=dev)
    w = torch.randn(8, 8, 3, 3, 3, device=dev) * 0.1
    for bad_x, bad_w in ((torch.randn(1, 4, 3, 4, 5, device=dev), torch.randn(4, 4, 3, 3, 3, device=dev)),
                         (x, torch.randn(8, 8, 1, 1, 1, device=dev)), (x, torch.randn(16, 8, 3, 3, 3, device=dev)),
                         (x[0], w)):
        with pytest.raises(ValueError, match="conv3d_k3: "):
            diffops.conv3d_k3(bad_x, bad_w)
    with pytest.raises(ValueError, match=r"\(8, 16, 32\)"):
        diffops.conv3d_k3(torch.randn(1, 4, 3, 4, 5, device=dev), torch.randn(4, 4, 3, 3, 3, device=dev))
    big = w.clone()
    big[2, 3, 1, 1, 1] = 9.0
    with pytest.raises(ValueError, match="split range"):
        diffops.conv3d_k3(x, big, check_weight=True)
    big[2, 3, 1, 1, 1] = 16.0   # 2^12 w leaves f16's range: hi = inf, lo = -inf
    assert not bool(diffops.conv3d_k3(x, big).isfinite().all())   # loud, not refused: no host sync on this path
    assert bool(diffops.conv3d_k3(x, w, check_weight=True).isfinite().all())

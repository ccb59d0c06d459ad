"""tests/volume_close_ref.py against the modules it restates, in float64 on the CPU: blocks.BasicConv's
norm + act, blocks.DoubleFeatureAtt's multiply, hourglass_ref.T, the closed-form gradients the HIP
backward implements, and the input builder's distance from the LeakyReLU kink."""
import pytest
import torch

import hourglass_ref as HR
import volume_close_ref as R
from stereoanywhere_amd import blocks


def test_matches_basicconv_and_feature_att():
    torch.manual_seed(3)
    B, C, D, H, W, FC = 2, 4, 6, 5, 7, 3
    bc = blocks.BasicConv(C, C, True, kernel_size=3, padding=1).double().eval()   # eval: instance statistics still
    att = blocks.DoubleFeatureAtt(C, FC).double()
    x = torch.randn(B, C, D, H, W, dtype=torch.float64)
    fl, fr = torch.randn(B, FC, H, W, dtype=torch.float64), torch.randn(B, FC, H, D, dtype=torch.float64)
    with torch.no_grad():
        y = bc.conv(x)
        gl, gr = torch.sigmoid(att.feat_att_left(fl)), torch.sigmoid(att.feat_att_right(fr))
        want = att(bc(x), fl, fr)
        assert torch.allclose(R.close(y), bc(x), rtol=0, atol=1e-13)
        assert torch.allclose(R.close(y, gl, gr), want, rtol=0, atol=1e-13)
        assert bc.act_fn.negative_slope == R.SLOPE and bc.norm_fn.eps == R.EPS and not bc.norm_fn.affine


@pytest.mark.parametrize("gated", (False, True))
def test_matches_hourglass_ref_T(gated):
    c = R.case(R.SHAPES[0], gated)
    x = c["x"].double()
    norm = R.stats(x)
    got = HR.T(x, norm, act=True, gate=(c["gl"], c["gr"]) if gated else None, slope=R.SLOPE)
    assert torch.allclose(got, c["ref"]["out"], rtol=0, atol=1e-13)
    mean, rstd = HR.stats(x)
    assert torch.allclose(mean, c["ref"]["mean"], rtol=0, atol=1e-14)
    assert torch.allclose(rstd, c["ref"]["rstd"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_closed_form_gradients(shape):
    """The formulas of csrc/volume_close.hip in float64 equal autograd's gradients."""
    c = R.case(shape, True)
    B, C, D, H, W = shape
    n = D * H * W
    x, g, gl, gr = (c[k].double() for k in ("x", "g", "gl", "gr"))
    xh = R.xhat(x)
    k = torch.where(xh > 0, torch.ones_like(xh), torch.full_like(xh, R.SLOPE))
    G = R.gate(gl, gr)
    u = g * G * k
    s1, s2 = u.sum((2, 3, 4), keepdim=True), (u * xh).sum((2, 3, 4), keepdim=True)
    rstd = c["ref"]["rstd"].reshape(B, C, 1, 1, 1)
    ga = g * xh * k
    ref = c["ref"]
    assert torch.allclose(rstd * (u - s1 / n - xh * s2 / n), ref["dx"], rtol=0, atol=1e-12)
    assert torch.allclose((ga * gr.permute(0, 1, 3, 2)[..., None]).sum(2), ref["dgl"], rtol=0, atol=1e-12)
    assert torch.allclose((ga * gl[:, :, None]).sum(4).permute(0, 1, 3, 2), ref["dgr"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_builder_stays_off_the_kink(shape):
    assert float(R.xhat(R.build_x(0, shape)).abs().min()) >= R.KINK
    for gated in (False, True):
        assert float(R.xhat(R.case(shape, gated)["x"]).abs().min()) >= R.KINK


def test_allowances_are_fp32_sized():
    """4 x torch's own fp32 deviation: a few 1e-7 at these shapes, never a loose bound."""
    for shape in R.SHAPES:
        for gated in (False, True):
            c = R.case(shape, gated)
            for key in ("out", "dx"):
                assert 0 < R.allowance(c, key) < 2e-6, (shape, gated, key, R.allowance(c, key))

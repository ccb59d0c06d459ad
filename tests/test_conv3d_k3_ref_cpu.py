"""tests/conv3d_k3_ref.py against the module and torch: the reference is blocks.BasicConv's own conv, the data
gradient is a plain conv with the flipped, channel-swapped weight (pinned to F.conv_transpose3d), the
[Cin][27][Cout] arrangement of dw is autograd's weight gradient, and the scale rule's numpy restatement is the
documented formula."""
import numpy as np
import pytest
import torch

import conv3d_k3_ref as R
from stereoanywhere_amd import blocks

F = torch.nn.functional


def _small(C=8, B=2, D=4, H=5, W=6, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(B, C, D, H, W, generator=gen, dtype=torch.float64),
            torch.randn(C, C, 3, 3, 3, generator=gen, dtype=torch.float64),
            torch.randn(B, C, D, H, W, generator=gen, dtype=torch.float64))


def test_reference_is_the_modules_conv():
    torch.manual_seed(0)
    m = blocks.BasicConv(8, 8, is_3d=True, kernel_size=3, stride=1, padding=1).double()
    x = torch.randn(1, 8, 4, 5, 6, dtype=torch.float64)
    assert m.conv.bias is None and tuple(m.conv.weight.shape) == (8, 8, 3, 3, 3)
    assert torch.equal(R.conv(x, m.conv.weight), m.conv(x))


def test_dx_is_a_conv_with_the_flipped_swapped_weight():
    x, w, g = _small()
    dx, _ = R.grads(x, w, g)
    by_conv = R.conv(g, R.flipped(w))
    torch.testing.assert_close(by_conv, F.conv_transpose3d(g, w, padding=1), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(by_conv, dx, rtol=1e-13, atol=1e-13)


def test_dw_arrangement():
    """dw[ci][tap][co] = sum x[b, ci, p + tap - 1] g[b, co, p], tap = (kd * 3 + kh) * 3 + kw."""
    x, w, g = _small(C=8, B=2, D=3, H=4, W=5)
    _, dw = R.grads(x, w, g)
    taps = R.to_taps(dw)
    assert tuple(taps.shape) == (8, 27, 8)
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    for tap in (0, 5, 13, 26):
        kd, kh, kw = tap // 9, tap // 3 % 3, tap % 3
        want = torch.einsum("bidhw,bodhw->io", xp[:, :, kd:kd + 3, kh:kh + 4, kw:kw + 5], g)
        torch.testing.assert_close(taps[:, tap, :], want, rtol=1e-12, atol=1e-12)
    assert torch.equal(R.from_taps(taps), dw)


@pytest.mark.parametrize("amax", [1.0, 3.0, 2.0 ** 13, 2.0 ** 14 - 1, 2.0 ** 14, 1e-25, 6e4, 1e20, 2.0 ** -40, 7e-7])
def test_scale_rule_brings_the_maximum_into_range(amax):
    k = R.scale_exponent(amax)
    assert k == 14 - (int(np.floor(np.log2(np.float64(np.float32(amax))))) + 1)   # the documented formula
    scaled = np.ldexp(np.float64(np.float32(amax)), k)
    assert 2.0 ** 13 <= scaled < 2.0 ** 14


def test_scale_rule_edges():
    assert [R.scale_exponent(v) for v in (0.0, np.inf, np.nan)] == [0, 0, 0]
    assert R.scale_exponent(1e-38) == 100 and R.scale_exponent(3e38) == -100   # the clamp
    t = torch.zeros(5, 2, 3)
    t[1, 0, 0], t[2, 1, 2], t[3, 0, 1], t[4, 1, 1] = -3.0, float("inf"), float("nan"), 2.0 ** -20
    assert R.sample_scales(t).tolist() == [1.0, 2.0 ** 12, 1.0, 1.0, 2.0 ** 33]


def test_cases_are_shared_and_cover_the_issues_shapes():
    assert R.case(*R.SHAPES[1]) is R.case(*R.SHAPES[1])
    assert len(R.SHAPES) == 6 and {s[0] for s in R.SHAPES} == {8, 16, 32}
    c = R.case(*R.SHAPES[1])
    assert c["dw"].shape == c["weight"].shape and bool((c["mag"] >= c["dw"].abs() - 1e-12).all())

"""The closed-form gradients that csrc/diffops_backward.hip implements (tests/diffops_ref.py, numpy
float64) against torch.autograd of the reference formulation in float64 on the CPU: the formulas the
kernels implement are the reference's."""
import numpy as np
import pytest
import torch

import diffops_ref as ref


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("W1,W2", [(13, 13), (9, 14)])
@pytest.mark.parametrize("use", [(1, 1, 1, 1), (1, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 1)])
def test_softargmin_closed_form_matches_autograd(W1, W2, use):
    """max |a - b| / max |b| <= 1e-12: both sides are float64 sums of a few dozen terms."""
    B, H = 2, 3
    rng = np.random.default_rng(5)
    vd = 4.0 * rng.standard_normal((B, H, W1, W2))
    vc = 4.0 * rng.standard_normal((B, H, W1, W2))
    vc[0, 0, 2, :] = 0.5      # a constant row: uniform softmax
    vc[1, 1, 3, 4] += 60.0    # one logit far above the rest: p -> 1
    g = [rng.standard_normal((B, H, n)) if u else None for u, n in zip(use, (W1, W2, W1, W2))]
    want = ref.softargmin_grads(vd, vc, g, torch.float64)
    got = ref.closed_softargmin(vd, vc, g)
    for name, a, b in zip(("grad_vol_disp", "grad_vol_conf"), got, want):
        assert (a is None) == (b is None), name
        if b is not None:
            print(f"{name}: relative difference {_rel(a, b):.3g}")
            assert _rel(a, b) <= 1e-12, name
            assert np.abs(b).max() > 0


@pytest.mark.parametrize("H,W,f", [(1, 1, 4), (5, 7, 4), (5, 7, 2), (4, 3, 1), (3, 4, 8)])
@pytest.mark.parametrize("use_scale", [True, False])
def test_convex_closed_form_matches_autograd(H, W, f, use_scale):
    B = 2
    rng = np.random.default_rng(7)
    flow = 10.0 * rng.standard_normal((B, 1, H, W))
    mask = 3.0 * rng.standard_normal((B, 9 * f * f, H, W))
    gout = rng.standard_normal((B, 1, f * H, f * W))
    want = ref.convex_grads(flow, mask, gout, f, use_scale, torch.float64)
    got = ref.closed_convex(flow, mask, gout, f, float(f) if use_scale else 1.0)
    for name, a, b in zip(("grad_flow", "grad_mask"), got, want):
        print(f"{name}: relative difference {_rel(a, b):.3g}")
        assert a.shape == b.shape and _rel(a, b) <= 1e-12, name


def test_forward_restatements():
    """The restated forwards against direct sums (float64): index conventions of the five formulas."""
    rng = np.random.default_rng(1)
    v = torch.from_numpy(rng.standard_normal((1, 2, 5, 6)))
    p = torch.softmax(v, 3)
    q = torch.softmax(v, 2)
    dL, dR = ref.left_disparity(v), ref.right_disparity(v)
    assert dL.shape == (1, 2, 5) and dR.shape == (1, 2, 6)
    assert abs(float(dL[0, 1, 3]) - (3 - sum(float(p[0, 1, 3, k]) * k for k in range(6)))) < 1e-12
    assert abs(float(dR[0, 1, 4]) - (sum(float(q[0, 1, j, 4]) * j for j in range(5)) - 4)) < 1e-12
    cL, cR = ref.left_confidence(v), ref.right_confidence(v)
    ent = -sum(float(p[0, 0, 2, k]) * np.log2(float(p[0, 0, 2, k]) + 1e-6) for k in range(6))
    assert abs(float(cL[0, 0, 2]) - (1 - ent / np.log2(6))) < 1e-12
    ent = -sum(float(q[0, 0, j, 1]) * np.log2(float(q[0, 0, j, 1]) + 1e-6) for j in range(5))
    assert abs(float(cR[0, 0, 1]) - (1 - ent / np.log2(5))) < 1e-12
    # up-sampling: output pixel (h f + a, w f + b) mixes the 3x3 neighbourhood of (h, w) with the
    # softmax of channels t f f + a f + b
    f, H, W = 2, 3, 4
    flow = torch.from_numpy(rng.standard_normal((1, 1, H, W)))
    mask = torch.from_numpy(rng.standard_normal((1, 9 * f * f, H, W)))
    up = ref.convex_upflow(flow, mask, f)
    h, w, a, b = 0, 3, 1, 0
    s = torch.softmax(mask[0, [t * f * f + a * f + b for t in range(9)], h, w], 0)
    want = 0.0
    for t in range(9):
        y, x = h + t // 3 - 1, w + t % 3 - 1
        if 0 <= y < H and 0 <= x < W:
            want += float(s[t]) * f * float(flow[0, 0, y, x])
    assert abs(float(up[0, 0, h * f + a, w * f + b]) - want) < 1e-12

"""tests/hourglass_ref.py (the float64 reference the per-kernel GPU tests of
tests/test_gpu_hourglass_ref.py rest on) against the torch Hourglass module in float64: the stage
functions chained in the order of Hourglass._forward_fused, with the weight slicing of
Hourglass.fused_weights restated here, reproduce the module's torch path plus the classifier conv.
Reference: hourglass.py:13-91, stereoanywhere.py:165-166."""
import numpy as np
import torch

import hourglass_ref as H
from stereoanywhere_amd.blocks import Hourglass


def _k3(w):   # [Cout, Cin, 3, 3, 3] -> [Cin][27][Cout]
    return w.reshape(w.shape[0], w.shape[1], 27).permute(1, 2, 0).contiguous()


def _gate(att, fl, fr):
    return torch.sigmoid(att.feat_att_left(fl)), torch.sigmoid(att.feat_att_right(fr))


def test_stage_chain_matches_torch_hourglass():
    B, D, Hh, W = 1, 12, 8, 16
    torch.manual_seed(0)
    hg = Hourglass(8, 8).double().eval()
    rng = np.random.default_rng(5)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    x = t(rng.standard_normal((B, 8, D, Hh, W)))
    fl = [t(rng.random((B, 1, Hh >> i, W >> i))) for i in range(4)]
    fr = [t(rng.random((B, 1, Hh >> i, D >> i))) for i in range(4)]
    wcls = t(rng.standard_normal((2, 8, 3, 3, 3)) * 0.2)
    with torch.no_grad():
        want = torch.nn.functional.conv3d(hg(x, fl, fr), wcls, padding=1)

        def layer(tx, conv, stride=1):   # BasicConv3d: the raw conv output + its InstanceNorm statistics
            y, _ = H.conv3(tx, _k3(conv.conv.weight), stride)
            return y, H.stats(y, conv.norm_fn.eps)
        slope = hg.final_agg[0].act_fn.negative_slope
        y, n = layer(H.T(x), hg.down_layers[0][0], 2)
        y, n = layer(H.T(y, n, True, None, slope), hg.down_layers[0][1])
        down0 = (y, n, True, _gate(hg.feature_atts[0], fl[1], fr[1]), slope)
        y, n = layer(H.T(*down0), hg.down_layers[1][0], 2)
        y, n = layer(H.T(y, n, True, None, slope), hg.down_layers[1][1])
        down1 = (y, n, True, _gate(hg.feature_atts[1], fl[2], fr[2]), slope)
        # agg_layers[1][0] over cat(up(down1) [32], down0 [16]); final_agg[0] over cat(orig [8], up(x) [16])
        a10 = hg.agg_layers[1][0].conv.weight.reshape(16, 48)
        y, _ = H.upcat(H.T(*down0), H.T(*down1), a10[:, 32:48].t(), a10[:, 0:32].t())
        n = H.stats(y)
        y, n = layer(H.T(y, n, True, None, slope), hg.agg_layers[1][1])
        y, n = layer(H.T(y, n, True, None, slope), hg.agg_layers[1][2])
        up1 = (y, n, True, _gate(hg.feature_atts_up[1], fl[1], fr[1]), slope)
        fa0 = hg.final_agg[0].conv.weight.reshape(8, 24)
        y, _ = H.upcat(H.T(x), H.T(*up1), fa0[:, 0:8].t(), fa0[:, 8:24].t())
        n = H.stats(y)
        y, n = layer(H.T(y, n, True, None, slope), hg.final_agg[1])
        y, n = layer(H.T(y, n, True, None, slope), hg.final_agg[2])
        last = H.T(y, n, True, _gate(hg.final_feature_atts_up, fl[0], fr[0]), slope)
        got, mag = H.conv3(last, _k3(wcls))
    assert got.shape == want.shape == (B, 2, D, Hh, W)
    err = float((got - want).abs().max())
    print(f"stage chain vs torch Hourglass (float64): max |diff| {err:.3g} at output scale {float(want.abs().max()):.3g}")
    assert err <= 1e-12
    assert bool((mag >= got.abs() * (1 - 1e-12)).all())   # the magnitude dominates the value


def test_upcat_range_and_magnitudes():
    """upcat's magnitudes: |out| <= a + p <= a + pm, and the per-axis steps of the corners (a constant
    low-resolution branch has none; a ramp along W has its slope along W and none along D, H)."""
    rng = np.random.default_rng(1)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ta, tu = t(rng.standard_normal((2, 8, 9, 6, 13))), t(rng.standard_normal((2, 16, 3, 2, 5)))
    wa, wu = t(rng.standard_normal((8, 8))), t(rng.standard_normal((16, 8)))
    out, m = H.upcat(ta, tu, wa, wu)
    assert bool((out.abs() <= (m["a"] + m["p"]) * (1 + 1e-12)).all()) and bool((m["p"] <= m["pm"] * (1 + 1e-12)).all())
    assert m["n"] == (3, 2, 5) and all(r.shape == out.shape and bool((r > 0).all()) for r in m["range"])
    _, m0 = H.upcat(ta, torch.ones_like(tu), wa, wu)
    assert max(float(r.abs().max()) for r in m0["range"]) < 1e-12
    ramp = torch.arange(5, dtype=torch.float64).expand(2, 16, 3, 2, 5)
    _, m1 = H.upcat(ta, ramp, wa, wu)
    slope = wu.sum(0).abs().reshape(1, 8, 1, 1, 1)
    assert float(m1["range"][0].max()) < 1e-12 and float(m1["range"][1].max()) < 1e-12
    assert float((m1["range"][2] - slope).abs().max()) < 1e-12

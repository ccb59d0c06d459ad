"""The hourglass with its two joins on diffops.upcat_conv (blocks.Hourglass(closes="hip", joins="hip"),
diffops.hourglass_forward(joins="hip")) against the same graph on torch in float64 on the CPU, on the
fixtures, shapes, seeds and metric of tests/test_gpu_volume_close_autograd.py: per tensor
max |got - ref64| / max |ref64| <= 4 x the same metric of the torch graph in fp32 on the CPU.  The kink
margins those seeds were chosen for belong to the float64 graph, which the joins do not change."""
import copy

import pytest
import torch
import torch.nn as nn

from stereoanywhere_amd import blocks, diffops
from test_gpu_volume_close_autograd import DEAD, FC, MARGIN, _graph, compare, hourglass  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture
def joins_taken(monkeypatch):
    """Counts the joins that ran on upcat_conv."""
    taken = []
    real = diffops.upcat_conv

    def counting(*a, **kw):
        taken.append(a[3] if len(a) > 3 else kw["low_first"])
        return real(*a, **kw)
    monkeypatch.setattr(diffops, "upcat_conv", counting)
    return taken


class _ReferenceLayout(nn.Module):
    """hourglass_forward(layout="reference", joins="hip") between the volume layout's permutes."""

    def __init__(self, hg):
        super().__init__()
        self.hg = hg

    def forward(self, x, fl, fr):
        out = diffops.hourglass_forward(self.hg, x.permute(0, 1, 3, 4, 2), fl, fr, joins="hip")   # [B,C,H,W1,W2]
        return out.permute(0, 1, 4, 2, 3)


def test_hourglass_joins_hip(hourglass, joins_taken):
    h = hourglass
    assert h["dist"] >= MARGIN
    got = _graph(h["hg"], h["inputs"], h["g"], torch.float32, "cuda", closes="hip", joins="hip")
    assert joins_taken == [True, False]
    compare("blocks.Hourglass(closes='hip', joins='hip')", got, h["ref"], h["f32"])
    for k, v in got[1].items():
        assert (v is None) == k.startswith(DEAD), k


def test_hourglass_forward_reference_layout_joins_hip(hourglass, joins_taken):
    h = hourglass
    out, grads = _graph(_ReferenceLayout(h["hg"]), h["inputs"], h["g"], torch.float32, "cuda")
    assert joins_taken == [True, False]
    compare("hourglass_forward(layout='reference', joins='hip')", (out, {k[3:]: v for k, v in grads.items()}),
            h["ref"], h["f32"])


def _on_gpu(h):
    hg = copy.deepcopy(h["hg"]).cuda()
    x, fl, fr = h["inputs"]
    return hg, x.cuda(), [f.cuda() for f in fl], [f.cuda() for f in fr]


def test_unbuilt_joins_fall_back_to_torch(joins_taken):
    torch.manual_seed(4)
    hg = blocks.Hourglass(4, 4, feature_channels=FC).cuda()
    x = torch.randn(1, 4, 16, 8, 16, device="cuda")
    fl = [torch.randn(1, FC[2 + i], 8 >> i, 16 >> i, device="cuda") for i in range(3)]
    fr = [torch.randn(1, FC[2 + i], 8 >> i, 16 >> i, device="cuda") for i in range(3)]
    with torch.no_grad():
        assert torch.equal(hg(x, fl, fr, closes="hip", joins="hip"), hg(x, fl, fr, closes="hip"))
    assert joins_taken == []


def test_bad_joins_values(hourglass):
    hg, x, fl, fr = _on_gpu(hourglass)
    with torch.no_grad():
        with pytest.raises(ValueError, match="joins must be"):
            hg(x, fl, fr, closes="hip", joins="triton")
        with pytest.raises(ValueError, match="joins must be"):
            diffops.hourglass_forward(hg, x, fl, fr, layout="volume", joins=None)
        with pytest.raises(ValueError, match="goes with closes"):
            hg(x, fl, fr, joins="hip")


def test_default_is_closes_hip_alone(hourglass, joins_taken):
    """The default call returns the bits of closes="hip" as it was: the joins' torch ops, restated here."""
    hg, x, fl, fr = _on_gpu(hourglass)
    F = torch.nn.functional
    with torch.no_grad():
        want = hg(x, fl, fr, closes="hip")
        assert torch.equal(want, hg(x, fl, fr, closes="hip", joins=None))
        assert torch.equal(want, diffops.hourglass_forward(hg, x, fl, fr, layout="volume"))
        assert torch.equal(want, diffops.hourglass_forward(hg, x, fl, fr, layout="volume", joins="torch"))
        assert joins_taken == []
        # the path before the keyword existed, op by op
        downs, y = [], x
        for i in range(2):
            y = diffops._close_gated(hg.down_layers[i], hg.feature_atts[i], y, fl[i + 1], fr[i + 1])
            downs.append(y)
        up = F.interpolate(downs[1], size=downs[0].shape[2:], mode="trilinear", align_corners=True)
        y = diffops._close_gated(hg.agg_layers[1], hg.feature_atts_up[1], torch.cat((up, downs[0]), 1), fl[1], fr[1])
        up = F.interpolate(y, size=x.shape[2:], mode="trilinear", align_corners=True)
        y = diffops._close_gated(hg.final_agg, hg.final_feature_atts_up, torch.cat((x, up), 1), fl[0], fr[0])
        assert torch.equal(want, y)
        got = hg(x, fl, fr, closes="hip", joins="hip")
        assert joins_taken == [True, False] and not torch.equal(got, want)   # another evaluation order

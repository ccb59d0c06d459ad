"""diffops.volume_close under autograd and the hourglass built on it (diffops.hourglass_forward,
blocks.Hourglass(closes="hip")) against the same graph on torch in float64 on the CPU.

Metric per tensor: max |got - ref64| / max |ref64|; allowed is 4 x the same metric of the torch graph in
fp32 on the CPU (computed here on the same seeded modules and inputs): the HIP closes make the same
handful of fp32 roundings per cell as torch's, in another order, and the convs are torch's on both
sides.  The seeds are chosen (on the CPU, from the float64 graph alone) so that no normalised value of
any InstanceNorm lies within MARGIN of the LeakyReLU kink, which each test asserts: an fp32 graph whose
conv output lands on the other side of the kink has a different, equally valid gradient there."""
import copy

import pytest
import torch
import torch.nn as nn

from stereoanywhere_amd import blocks, diffops

pytestmark = pytest.mark.gpu

MARGIN = 5e-5
FC = (1, 1, 4, 6, 8, 8)   # feature channels; the hourglass uses levels 2.. of them
# (volume D, H, W; the feature pyramid's base D, H, W; seed): multiples of 4 with a matching pyramid (every
# gate fused), and 18 x 8 x 18 on the 16 x 8 x 16 pyramid (every gate resized: the gate-less close + torch)
FUSED = ((16, 8, 16), (16, 8, 16), 73)
RESIZED = ((18, 8, 18), (16, 8, 16), 270)


def metric(got, ref):
    return float((got.double().cpu() - ref.double()).abs().max() / ref.double().abs().max())


def kink_distance(module, call):
    """min |xh| over every InstanceNorm output of one forward of `module` (float64 on the CPU)."""
    seen = []
    hooks = [m.register_forward_hook(lambda _m, _i, o: seen.append(float(o.abs().min())))
             for m in module.modules() if isinstance(m, (nn.InstanceNorm2d, nn.InstanceNorm3d))]
    with torch.no_grad():
        call()
    for h in hooks:
        h.remove()
    return min(seen)


def compare(name, got, ref, f32):
    """got / ref / f32: (output, {parameter name: grad or None})."""
    worst = {}
    for key in ["out"] + sorted(ref[1]):
        g, r, f = (t[0] if key == "out" else t[1][key] for t in (got, ref, f32))
        if r is None:
            assert g is None, f"{name}: {key} is dead and must have no gradient"
            continue
        assert g is not None, f"{name}: {key} has no gradient"
        m, allowed = metric(g, r), 4.0 * metric(f, r)
        worst[key] = (m, allowed)
        assert m <= allowed, (name, key, m, allowed)
    key = max(worst, key=lambda k: worst[k][0] / worst[k][1])
    print(f"{name}: closest to its allowance: {key} deviates {worst[key][0]:.3g}, allowed {worst[key][1]:.3g}")


# --------------------------------------------------------------------------- a small graph
class Small(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv3d(3, 4, 3, padding=1, bias=False)
        self.left, self.right = nn.Conv2d(5, 4, 1), nn.Conv2d(5, 4, 1)
        self.norm = nn.InstanceNorm3d(4)

    def forward(self, v, fl, fr, hip=False):
        y, gl, gr = self.conv(v), torch.sigmoid(self.left(fl)), torch.sigmoid(self.right(fr))
        if hip:
            return diffops.volume_close(y, gl, gr)
        y = torch.nn.functional.leaky_relu(self.norm(y), 0.01)
        return y * gl[:, :, None] * gr.permute(0, 1, 3, 2)[..., None]


def _graph(module, inputs, g, dtype, device, **kw):
    m = copy.deepcopy(module).to(device=device, dtype=dtype)
    out = m(*[[f.to(device=device, dtype=dtype) for f in t] if isinstance(t, list) else t.to(device=device, dtype=dtype)
              for t in inputs], **kw)
    (out * g.to(device=device, dtype=dtype)).sum().backward()
    return out.detach().cpu(), {k: None if p.grad is None else p.grad.cpu() for k, p in m.named_parameters()}


def test_volume_close_in_a_small_graph():
    torch.manual_seed(11)
    m = Small()
    v, fl, fr = torch.randn(1, 3, 6, 5, 7), torch.randn(1, 5, 5, 7), torch.randn(1, 5, 5, 6)
    g = torch.randn(1, 4, 6, 5, 7)
    m64 = copy.deepcopy(m).double()
    assert kink_distance(m64, lambda: m64(v.double(), fl.double(), fr.double())) >= MARGIN
    ref = _graph(m, (v, fl, fr), g, torch.float64, "cpu")
    f32 = _graph(m, (v, fl, fr), g, torch.float32, "cpu")
    got = _graph(m, (v, fl, fr), g, torch.float32, "cuda", hip=True)
    compare("small graph", got, ref, f32)


# --------------------------------------------------------------------------- the hourglass
def build(size, base, seed):
    torch.manual_seed(seed)
    hg = blocks.Hourglass(8, 8, feature_channels=FC)
    D, H, W = size
    x, g = torch.randn(1, 8, D, H, W), torch.randn(1, 8, D, H, W)
    fl = [torch.randn(1, FC[2 + i], base[1] >> i, base[2] >> i) for i in range(3)]
    fr = [torch.randn(1, FC[2 + i], base[1] >> i, base[0] >> i) for i in range(3)]
    return hg, (x, fl, fr), g


class _ReferenceLayout(nn.Module):
    """hourglass_forward(layout="reference") between the volume layout's permutes."""

    def __init__(self, hg):
        super().__init__()
        self.hg = hg

    def forward(self, x, fl, fr):
        out = diffops.hourglass_forward(self.hg, x.permute(0, 1, 3, 4, 2), fl, fr)   # [B,C,H,W1,W2]
        return out.permute(0, 1, 4, 2, 3)


@pytest.fixture(scope="module", params=(FUSED, RESIZED), ids=("fused-16x8x16", "resized-18x8x18"))
def hourglass(request):
    hg, inputs, g = build(*request.param)
    h64 = copy.deepcopy(hg).double()
    dist = kink_distance(h64, lambda: h64(inputs[0].double(), *[[f.double() for f in t] for t in inputs[1:]]))
    return dict(hg=hg, inputs=inputs, g=g, dist=dist, ref=_graph(hg, inputs, g, torch.float64, "cpu"),
                f32=_graph(hg, inputs, g, torch.float32, "cpu"))


DEAD = ("down_layers.2.", "feature_atts.2.", "agg_layers.0.", "feature_atts_up.0.")


def test_hourglass_reference_setup(hourglass):
    assert hourglass["dist"] >= MARGIN
    for k, v in hourglass["ref"][1].items():
        assert (v is None) == k.startswith(DEAD), k


def test_hourglass_closes_hip(hourglass):
    h = hourglass
    got = _graph(h["hg"], h["inputs"], h["g"], torch.float32, "cuda", closes="hip")
    compare("blocks.Hourglass(closes='hip')", got, h["ref"], h["f32"])


def test_hourglass_forward_reference_layout(hourglass):
    h = hourglass
    out, grads = _graph(_ReferenceLayout(h["hg"]), h["inputs"], h["g"], torch.float32, "cuda")
    compare("hourglass_forward(layout='reference')", (out, {k[3:]: v for k, v in grads.items()}), h["ref"], h["f32"])


def test_hourglass_forward_volume_layout_is_the_module_path(hourglass):
    hg = copy.deepcopy(hourglass["hg"]).cuda()
    x, fl, fr = hourglass["inputs"]
    x, fl, fr = x.cuda(), [f.cuda() for f in fl], [f.cuda() for f in fr]
    with torch.no_grad():
        assert torch.equal(diffops.hourglass_forward(hg, x, fl, fr, layout="volume"), hg(x, fl, fr, closes="hip"))
        with pytest.raises(ValueError, match="layout must be"):
            diffops.hourglass_forward(hg, x, fl, fr, layout="nchw")
        with pytest.raises(ValueError, match="closes must be"):
            hg(x, fl, fr, closes="triton")


def test_default_path_is_unchanged(hourglass):
    hg = copy.deepcopy(hourglass["hg"]).cuda()
    x, fl, fr = hourglass["inputs"]
    x, fl, fr = x.cuda(), [f.cuda() for f in fl], [f.cuda() for f in fr]
    with torch.no_grad():
        assert torch.equal(hg(x, fl, fr), hg(x, fl, fr, closes=None))
        assert torch.equal(hg(x, fl, fr), hg(x, fl, fr, None, None))

"""forward(test_mode=False): the reference's six-element tuple (stereoanywhere.py:299), evaluated
without gradients, against the reference run with the same seeded weights and
volume_corruption_prob=0 (tests/golden/full_outputs.npz, written by
tests/golden/make_golden_full_outputs.py).

Gates.  Every iteration's prediction and the scale/shift-aligned mono depth: EPE < 1e-3, the
project's end-to-end gate.  The coarse mono / stereo disparities (+-65 with seeded weights) and the
mono confidence (4e-5 .. 1.4e-2) have no absolute gate that means something for both: they are held to
mean|ours - ref| / mean|ref| at four times the value measured on the MI355X, rounded up to one digit
and never looser than 1e-3 (REL_GATE; the measured values are in DESIGN.md 4d).
"""
import json

import numpy as np
import pytest
import torch

from fixtures_util import epe, load_fixture, regenerate_inputs
from mask_upsample_ref import reference as upsample_reference
from stereoanywhere_amd import ops, synth
from stereoanywhere_amd.graph import ForwardGraph
from stereoanywhere_amd.model import StereoAnywhere

pytestmark = pytest.mark.gpu

PUBLISHED = dict(use_truncate_vol=True, use_aggregate_mono_vol=True, vol_n_masks=8, n_additional_hourglass=0,
                 vol_downsample=0, mirror_conf_th=0.98, mirror_attenuation=0.9, lrc_th=1.0, normal_gain=10,
                 volume_corruption_prob=0)
CASES = ["published", "agg_stereo", "vd1", "gru1_L2r3"]
KEYS = ("left", "right", "mono_left", "mono_right")
# mean|ours - ref| / mean|ref|, the largest measured over all cases, both views and both kernel sets:
# dispmono 1.219e-7, dispstereo 1.259e-7, ldispmonoconf 8.119e-5 (vd1, view 2; 3.561e-5 without
# vol_downsample) -> x 4, rounded up to one digit
REL_GATE = {"coarse_dispmono": 5e-7, "coarse_dispstereo": 6e-7, "coarse_ldispmonoconf": 4e-4}


@pytest.fixture(scope="module")
def fix():
    torch.backends.cudnn.benchmark = False
    return load_fixture("full_outputs.npz")


@pytest.fixture(scope="module")
def pair(fix):
    H, W, seed = (int(v) for v in fix["shape"])
    return regenerate_inputs(fix, 1, H, W, float(fix["D"]), seed0=seed)


def build(fix, name):
    over = json.loads(str(fix[f"{name}.args"]))
    m = StereoAnywhere(dict(PUBLISHED, **over)).eval()
    synth.load_seeded_weights(m, 0)
    return m.cuda()


def tensors(pair):
    return [torch.from_numpy(pair[k]).cuda() for k in KEYS]


def full(model, x, iters):
    with torch.no_grad():
        return model(*x, iters=iters, test_mode=False)


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).mean() / np.abs(ref).mean())


@pytest.mark.parametrize("kernels", ["fp32", "split"])
@pytest.mark.parametrize("name", CASES)
def test_full_outputs_vs_reference(fix, pair, monkeypatch, name, kernels):
    """Every case of the fixture, 4 iterations, on the fp32 and the f16-split conv kernels: the
    tuple's structure, then every entry against the reference."""
    monkeypatch.setattr(ops, "W4_SPLIT", kernels != "fp32")
    monkeypatch.setattr(ops, "DIRECT_SPLIT", kernels != "fp32")
    iters = int(fix["iters"])
    x = tensors(pair)
    out = full(build(fix, name), x, iters)
    assert isinstance(out, tuple) and len(out) == 6
    flows, confs, c2, c3, l2, l3 = out
    assert isinstance(flows, list) and len(flows) == iters and confs == [None] * iters
    assert all(isinstance(v, list) and len(v) == 3 for v in (c2, c3, l2, l3))
    B, _, H, W = x[0].shape
    stereo = name == "agg_stereo"
    for view, coarse, conf in (("2", c2, l2), ("3", c3, l3)):
        assert conf[0] is None and conf[2] is None
        assert (coarse[0] is not None) == stereo
        assert (f"{name}.coarse_dispstereo{view}" in fix) == stereo
    tens = flows + [t for v in (c2, c3, l2, l3) for t in v if t is not None]
    for t in tens:
        assert t.shape == (B, 1, H, W) and t.dtype == torch.float32 and t.device == x[0].device
        assert not t.requires_grad and torch.isfinite(t).all()
    ref = fix[f"{name}.flow_predictions"]
    assert ref.shape == (iters, B, 1, H, W)
    for i, f in enumerate(flows):
        e = epe(f.cpu().numpy(), ref[i])
        print(f"{name} {kernels} iteration {i}: EPE {e:.3e}")
        assert e < 1e-3
    for view, coarse, conf in (("2", c2, l2), ("3", c3, l3)):
        e = epe(coarse[2].cpu().numpy(), fix[f"{name}.coarse_scaled_mde{view}"])
        print(f"{name} {kernels} coarse_scaled_mde{view}: EPE {e:.3e}")
        assert e < 1e-3
        for key, t in (("coarse_dispstereo", coarse[0]), ("coarse_dispmono", coarse[1]),
                       ("coarse_ldispmonoconf", conf[1])):
            if t is None:
                continue
            r = rel(t.cpu().numpy(), fix[f"{name}.{key}{view}"])
            print(f"{name} {kernels} {key}{view}: mean|d| / mean|ref| {r:.3e} (gate {REL_GATE[key]:.0e})")
            assert r < REL_GATE[key] <= 1e-3


def test_last_prediction_is_the_test_mode_output(fix, pair, monkeypatch):
    """fuse_mask_upsample=False issues the test-mode forward's launches for the last prediction: the
    same bits.  The default (one kernel) stays within the operator's bound of it
    (tests/test_gpu_mask_upsample.py), computed from the kernel's own inputs at the last iteration.
    A test-mode forward after the full-outputs forwards returns the bits it returned before them."""
    m = build(fix, "published")
    x = tensors(pair)
    iters = int(fix["iters"])
    with torch.no_grad():
        before = m(*x, iters=iters, test_mode=True)[0].clone()
    m.opts.fuse_mask_upsample = False
    unfused = full(m, x, iters)[0]
    assert torch.equal(unfused[-1], before)
    m.opts.fuse_mask_upsample = True
    seen = []
    real = ops.mask_upsample

    def spy(xm, ws, bias, scale, flow_x, out=None):
        seen.append((xm.clone(), bias, scale, flow_x.clone()))
        return real(xm, ws, bias, scale, flow_x, out=out)
    monkeypatch.setattr(ops, "mask_upsample", spy)
    fused = full(m, x, iters)[0]
    monkeypatch.setattr(ops, "mask_upsample", real)
    assert len(seen) == iters
    xm, bias, scale, flow_x = seen[-1]
    assert scale == 0.25
    _, bound = upsample_reference(xm, m.update_block.mask[2].weight.detach(), bias.detach(), scale, flow_x)
    d = (fused[-1].double() - before.double()).abs()
    print(f"fused last prediction vs test mode: max |d| {float(d.max()):.3e}, max d / bound "
          f"{float((d / bound).max()):.3f}, bit-identical {torch.equal(fused[-1], before)}")
    assert bool((d <= bound).all())
    for i in range(iters):   # every iteration, not only the last, agrees between the two paths
        assert epe(fused[i].cpu().numpy(), unfused[i].cpu().numpy()) < 1e-4
    with torch.no_grad():
        after = m(*x, iters=iters, test_mode=True)[0]
    assert torch.equal(after, before)


def test_batch_parts(fix):
    """B = 2 with loop_parts = 2 (each part writes its batch slice of every iteration's prediction):
    equal to its two B = 1 forwards at EPE < 1e-4 for every iteration, the batch-parts criterion."""
    m = build(fix, "published")
    m.opts.loop_parts = 2
    H, W, _ = (int(v) for v in fix["shape"])
    pb = synth.synthetic_batch(2, H, W, float(fix["D"]), seed0=1)
    iters = int(fix["iters"])
    out = full(m, tensors(pb), iters)
    flows = out[0]
    assert flows[0].shape == (2, 1, H, W) and flows[1].data_ptr() - flows[0].data_ptr() == 2 * H * W * 4
    for i in range(2):
        single = full(m, tensors({k: v[i:i + 1] for k, v in pb.items()}), iters)
        for it in range(iters):
            e = epe(flows[it][i:i + 1].cpu().numpy(), single[0][it].cpu().numpy())
            print("loop_parts=2 pair", i, "iteration", it, "EPE vs B=1", e)
            assert e < 1e-4
        for lst, ref in zip(out[2:], single[2:]):
            for a, b in zip(lst, ref):
                assert (a is None) == (b is None)
                if a is not None:
                    assert rel(a[i:i + 1].cpu().numpy(), b.cpu().numpy()) < 1e-5


def test_mixed_precision_full_outputs():
    """model.mixed_precision / torch.autocast run the full-outputs forward on the single-f16-operand
    kernels: every prediction within the mixed fixture's gate (the reference's own f16 autocast EPE on
    this input, tests/golden/mixed.npz) of the fp32 forward's."""
    mfix = load_fixture("mixed.npz")
    H, W, seed, iters = (int(v) for v in mfix["tiny.shape"])
    p = regenerate_inputs(mfix, 1, H, W, float(mfix["tiny.D"]), seed0=seed, prefix="tiny.")
    gate = float(mfix["tiny.epe_autocast_f16"])
    m = StereoAnywhere(dict(PUBLISHED)).eval()
    synth.load_seeded_weights(m, 0)
    m = m.cuda()
    x = tensors(p)
    f32 = full(m, x, iters)[0]
    m.mixed_precision = True
    mixed = full(m, x, iters)[0]
    m.mixed_precision = False
    with torch.autocast("cuda"), torch.no_grad():
        auto = m(*x, iters=iters, test_mode=False)[0]
    assert not torch.equal(mixed[-1], f32[-1])
    for i in range(iters):
        assert mixed[i].dtype == torch.float32 and torch.isfinite(mixed[i]).all()
        assert torch.equal(auto[i], mixed[i])
        e = epe(mixed[i].cpu().numpy(), f32[i].cpu().numpy())
        print(f"iteration {i}: EPE mixed vs fp32 {e:.3e} (gate {gate:.3e})")
        assert e <= gate


def test_forward_graph_keeps_refusing(fix, pair):
    m = build(fix, "published")
    with pytest.raises(NotImplementedError):
        ForwardGraph(m)(*tensors(pair), iters=2, test_mode=False)

"""End to end at model geometries other than the published one: 1..3 GRU levels, 1..4 pyramid
levels, lookup radius 1..8, against the reference run with the same seeded weights
(tests/golden/geometry.npz, written by tests/golden/make_golden_geometry.py)."""
import json

import numpy as np
import pytest
import torch

from fixtures_util import epe, load_fixture, regenerate_inputs
from stereoanywhere_amd import ops, synth
from stereoanywhere_amd.model import StereoAnywhere

pytestmark = pytest.mark.gpu

PUBLISHED = dict(use_truncate_vol=True, use_aggregate_mono_vol=True, vol_n_masks=8, n_additional_hourglass=0,
                 vol_downsample=0, mirror_conf_th=0.98, mirror_attenuation=0.9, lrc_th=1.0, normal_gain=10)
CASES = ["gru2", "gru1", "L2", "L1r1", "L3r2", "r8", "gru2_L2r3", "gru1_L4r6"]
KEYS = ("left", "right", "mono_left", "mono_right")


@pytest.fixture(scope="module")
def fix():
    torch.backends.cudnn.benchmark = False
    return load_fixture("geometry.npz")


@pytest.fixture(scope="module")
def pairs(fix):
    """The two inputs of the fixture, regenerated once (their digests are checked)."""
    out = {}
    for prefix in ("", "wide."):
        H, W, seed = (int(v) for v in fix[prefix + "shape"])
        out[prefix] = regenerate_inputs(fix, 1, H, W, float(fix[prefix + "D"]), seed0=seed, prefix=prefix)
    return out


def build(fix, name):
    over = json.loads(str(fix[f"{name}.args"]))
    m = StereoAnywhere(dict(PUBLISHED, **over)).eval()
    synth.load_seeded_weights(m, 0)
    return m.cuda()


def tensors(pair):
    return [torch.from_numpy(pair[k]).cuda() for k in KEYS]


def run(model, pair, iters):
    flow_up, none = model(*tensors(pair), iters=iters, test_mode=True)
    assert none is None
    return -flow_up[:, 0].cpu().numpy()


def run_counted(model, pair, iters, monkeypatch, split):
    monkeypatch.setattr(ops, "W4_SPLIT", split)
    monkeypatch.setattr(ops, "DIRECT_SPLIT", split)
    ops.WORK = {}
    try:
        disp = run(model, pair, iters)
        work = dict(ops.WORK)
    finally:
        ops.WORK = None
    assert work.get("corr_lookup", 0.0) > 0 and "conv2d_wino4" in work
    return disp


@pytest.mark.parametrize("kernels", ["fp32", "split"])
@pytest.mark.parametrize("name", CASES)
def test_geometry_vs_reference(fix, pairs, monkeypatch, name, kernels):
    """Every case of the table on the 64x128 input of tiny_64x128_it4.npz, 4 iterations: EPE against
    the reference < 1e-3 (the project's end-to-end gate), on the fp32 and the f16-split conv kernels."""
    iters = int(fix["iters"])
    disp = run_counted(build(fix, name), pairs[""], iters, monkeypatch, kernels != "fp32")
    ref = fix[f"{name}.disparity"]
    e = epe(disp, ref)
    print(name, kernels, "EPE", e, "max", float(np.abs(disp - ref).max()))
    assert np.isfinite(disp).all() and e < 1e-3


@pytest.mark.parametrize("kernels", ["fp32", "split"])
def test_ragged_96x160_vs_reference(fix, pairs, monkeypatch, kernels):
    """96x160: W/4 = 40 (level widths 40, 20, 10), W/16 = 10, a GRU plane whose width is no
    multiple of 4.  The published geometry first, on the same input: it shows that the input is
    well-conditioned for the reference's quantile-band least squares."""
    iters = int(fix["iters"])
    split = kernels != "fp32"
    base = run_counted(build(fix, "base_96x160"), pairs["wide."], iters, monkeypatch, split)
    e0 = epe(base, fix["base_96x160.disparity"])
    print("base_96x160", kernels, "EPE", e0)
    assert e0 < 1e-3
    disp = run_counted(build(fix, "gru2_L3r5_96x160"), pairs["wide."], iters, monkeypatch, split)
    ref = fix["gru2_L3r5_96x160.disparity"]
    e = epe(disp, ref)
    print("gru2_L3r5_96x160", kernels, "EPE", e, "max", float(np.abs(disp - ref).max()))
    assert np.isfinite(disp).all() and e < 1e-3


def test_forward_graph_replays_gru2_L2r3(fix, pairs):
    """graph.ForwardGraph captures a non-published geometry as it stands: the replay equals the
    eager forward bit for bit."""
    from stereoanywhere_amd.graph import ForwardGraph
    m = build(fix, "gru2_L2r3")
    x = tensors(pairs[""])
    with torch.no_grad():
        ref = m(*x, iters=4, test_mode=True)[0].clone()
        got = ForwardGraph(m)(*x, iters=4)[0]
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all()
    assert torch.equal(got, ref)


def test_loop_parts_gru1_L4r6(fix):
    """The GRU loop in two batch parts (the generator yields twice per iteration at one GRU
    level too): a B = 2 batch equals its two B = 1 forwards at EPE < 1e-4."""
    m = build(fix, "gru1_L4r6")
    m.opts.loop_parts = 2
    H, W, _ = (int(v) for v in fix["shape"])
    pb = synth.synthetic_batch(2, H, W, float(fix["D"]), seed0=1)
    batch = run(m, pb, 4)
    assert np.isfinite(batch).all()
    for i in range(2):
        single = run(m, {k: v[i:i + 1] for k, v in pb.items()}, 4)
        e = epe(batch[i:i + 1], single)
        print("gru1_L4r6 loop_parts=2 pair", i, "EPE vs B=1", e)
        assert e < 1e-4


def test_sheared_pipeline_equals_row_layout(fix, pairs):
    """opts.shear_min_bytes = 0 puts the small shape on the sheared pipeline (row pyramid, shear
    copy, sheared lookup at 3 levels of radius 2): the same bits as the row-layout run."""
    m = build(fix, "L3r2")
    assert ops.shear_supported(1, 16, 32, 32, 3)
    m.opts.shear_min_bytes = 0
    m.opts.sheared_lookup = True
    sheared = run(m, pairs[""], 4)
    m.opts.sheared_lookup = False
    row = run(m, pairs[""], 4)
    assert np.isfinite(row).all()
    assert np.array_equal(sheared, row)


def test_refusals(fix):
    """What stays unbuilt is refused with NotImplementedError: n_downsample=3 (where the reference
    itself raises IndexError), and at construction corr_levels=5 and n_downsample=1."""
    assert str(fix["nd3.error"]) == "IndexError"
    m = StereoAnywhere(dict(PUBLISHED, n_downsample=3)).eval().cuda()
    t = [torch.zeros(1, c, 64, 128, device="cuda") for c in (3, 3, 1, 1)]
    with pytest.raises(NotImplementedError, match="n_downsample=2"):
        m(*t, iters=1, test_mode=True)
    with pytest.raises(NotImplementedError, match="1..4 pyramid levels"):
        StereoAnywhere(dict(PUBLISHED, corr_levels=5))
    with pytest.raises(NotImplementedError, match="n_downsample=2"):
        StereoAnywhere(dict(PUBLISHED, n_downsample=1))

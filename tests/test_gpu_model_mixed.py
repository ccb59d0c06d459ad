"""StereoAnywhere in mixed precision (model.mixed_precision, or a call under torch.autocast("cuda")):
every split-eligible F(4x4,3x3) launch on the single-f16-operand kernel (block_shape 7), everything
else fp32, float32 out.

Accuracy contract (tests/golden/mixed.npz, made by make_golden_mixed.py from the reference): the mode
may not be further from the reference's fp32 disparity than the reference's own f16 autocast is
(margin x1; a CPU emulation of the mode predicted about one ninth of it)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fixtures_util import epe, load_fixture, regenerate_inputs
from stereoanywhere_amd import data, ops, synth, tiler
from stereoanywhere_amd.graph import ForwardGraph
from stereoanywhere_amd.model import StereoAnywhere

pytestmark = pytest.mark.gpu
PUBLISHED = dict(use_truncate_vol=True, use_aggregate_mono_vol=True, vol_n_masks=8, n_additional_hourglass=0,
                 vol_downsample=0, mirror_conf_th=0.98, mirror_attenuation=0.9, lrc_th=1.0, normal_gain=10)
KEYS = ("left", "right", "mono_left", "mono_right")


@pytest.fixture(scope="module")
def fix():
    return load_fixture("mixed.npz")


@pytest.fixture(scope="module")
def model():
    torch.backends.cudnn.benchmark = False
    m = StereoAnywhere(dict(PUBLISHED)).eval()
    synth.load_seeded_weights(m, 0)
    return m.cuda()


def _inputs(fix, name):
    H, W, seed, iters = (int(v) for v in fix[name + ".shape"])
    pair = regenerate_inputs(fix, 1, H, W, float(fix[name + ".D"]), seed0=seed, prefix=name + ".")
    return [torch.from_numpy(pair[k]).cuda() for k in KEYS], iters


def _forward(model, x, iters, mixed):
    """(flow_up, launches per block shape) of one forward with model.mixed_precision = mixed."""
    ops.W4_SHAPE_LAUNCHES.clear()
    model.mixed_precision = mixed
    try:
        out = model(*x, iters=iters, test_mode=True)[0]
    finally:
        model.mixed_precision = False
    return out, dict(ops.W4_SHAPE_LAUNCHES)


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_mixed_vs_reference_and_modes(model, fix, name):
    assert name in str(fix["cases"]).split(",")
    x, iters = _inputs(fix, name)
    ref32, bound = fix[name + ".disparity"], float(fix[name + ".epe_autocast_f16"])
    assert abs(epe(fix[name + ".disparity_autocast_f16"], ref32) - bound) < 1e-9
    d0, s0 = _forward(model, x, iters, False)
    dm, sm = _forward(model, x, iters, True)
    d2, s2 = _forward(model, x, iters, False)
    # launches: the mode moves every split launch to shape 7 and nothing else
    assert sm.get(7, 0) > 0 and sm.get(6, 0) == 0, sm
    assert s0.get(6, 0) > 0 and s0.get(7, 0) == 0, s0
    assert sm.get(7, 0) == s0.get(6, 0) and {k: v for k, v in sm.items() if k != 7} == \
        {k: v for k, v in s0.items() if k != 6}, (s0, sm)
    assert s2 == s0
    # no state leaks: default -> mixed -> default
    assert torch.equal(d0, d2)
    assert dm.dtype == torch.float32 and torch.isfinite(dm).all()
    assert not torch.equal(dm, d0)
    e_mixed = epe(-dm[:, 0].cpu().numpy(), ref32)
    e_default = epe(-d0[:, 0].cpu().numpy(), ref32)
    print(f"{name}: EPE vs the reference's fp32: mixed {e_mixed:.3e}, default {e_default:.3e}; "
          f"the reference's own f16 autocast {bound:.3e} (mixed / autocast {e_mixed / bound:.3f})")
    assert e_default < 1e-3
    assert e_mixed <= bound, (e_mixed, bound)
    # how the reference's harnesses ask: autocast
    ops.W4_SHAPE_LAUNCHES.clear()
    with torch.autocast("cuda"):
        da = model(*x, iters=iters, test_mode=True)[0]
    assert ops.W4_SHAPE_LAUNCHES == sm
    assert da.dtype == torch.float32 and torch.equal(da, dm)
    with torch.autocast("cuda", enabled=False):
        assert torch.equal(model(*x, iters=iters, test_mode=True)[0], d0)


def test_forward_graph_in_the_mode(model, fix):
    """A ForwardGraph captured in the mode replays bit-equal to the eager mixed forward; a graph
    captured in default mode is not replayed for a mixed call (the mode is in the capture key)."""
    x, iters = _inputs(fix, "tiny")
    d0, _ = _forward(model, x, iters, False)
    dm, _ = _forward(model, x, iters, True)
    fg = ForwardGraph(model)
    assert torch.equal(fg(*x, iters=iters)[0], d0)
    g_default = fg._graph
    with torch.autocast("cuda"):
        got = fg(*x, iters=iters)[0]
    assert fg._graph is not g_default            # captured again for the mixed call
    assert got.dtype == torch.float32 and torch.equal(got, dm)
    g_mixed = fg._graph
    model.mixed_precision = True                 # the attribute asks for the same capture
    try:
        assert torch.equal(fg(*x, iters=iters)[0], dm)
        assert fg._graph is g_mixed
    finally:
        model.mixed_precision = False
    assert torch.equal(fg(*x, iters=iters)[0], d0) and fg._graph is not g_mixed


def test_tile_wrapper_flag_reaches_the_kernels(model):
    """TileWrapper(batch_tiles=True) at the smallest tiling of test_gpu_tiled.py (200 x 260 in 96 x 128
    tiles, overlap 32): mixed_precision=True runs the tiles on shape 7, False on none."""
    H, W, th, tw, ov = 200, 260, 96, 128, 32
    p = synth.synthetic_batch(1, H, W, 32.0, seed0=2)
    x = [torch.from_numpy(p[k]).cuda() for k in KEYS]
    wrap = tiler.TileWrapper(model, tile_width=tw, tile_height=th, overlap=ov, batch_tiles=True)
    out = {}
    for flag in (True, False):
        ops.W4_SHAPE_LAUNCHES.clear()
        out[flag] = wrap(*x, mixed_precision=flag, iters=2, test_mode=True)
        s = dict(ops.W4_SHAPE_LAUNCHES)
        if flag:
            assert s.get(7, 0) > 0 and s.get(6, 0) == 0, s
        else:
            assert s.get(7, 0) == 0 and s.get(6, 0) > 0, s
        assert out[flag].shape == (1, 1, H, W) and out[flag].dtype == torch.float32
        assert torch.isfinite(out[flag]).all()
    assert not torch.equal(out[True], out[False])


def test_cli_mixed_precision_writes_the_mixed_forward(model, tmp_path):
    """test.py --mixed_precision on the synthetic dataset of test_gpu_cli.py: the written disparity is
    the mixed forward's (and not the default one's)."""
    import test as cli
    args = ["--dataset", "synthetic", "--synthetic_size", "120x250", "--synthetic_count", "1", "--iters", "4",
            "--monomodel", "synthetic", "--use_truncate_vol", "--use_aggregate_mono_vol", "--maxdisp", "48",
            "--outdir", str(tmp_path / "out"), "--mixed_precision"]
    ops.W4_SHAPE_LAUNCHES.clear()
    cli.main(args)
    s = dict(ops.W4_SHAPE_LAUNCHES)
    assert s.get(7, 0) > 0 and s.get(6, 0) == 0, s
    smp = data.SyntheticPairs(1, 120, 250, 48.0)[0]
    x = [torch.from_numpy(smp[k])[None].cuda() for k in ("im2", "im3", "im2_mono", "im3_mono")]
    lo, hi = torch.minimum(x[2].min(), x[3].min()), torch.maximum(x[2].max(), x[3].max())
    x[2], x[3] = (x[2] - lo) / (hi - lo), (x[3] - lo) / (hi - lo)
    pad = tiler.pad32(120, 250)
    xp = [F.pad(t, pad, mode="replicate") for t in x]
    written = data.read_pfm(str(tmp_path / "out" / "synthetic0_disp.pfm"))
    assert written.shape == (120, 250)
    d = {}
    for mixed in (True, False):
        o = -_forward(model, xp, 4, mixed)[0][0, 0]
        d[mixed] = o[pad[2]:o.shape[0] - pad[3], pad[0]:o.shape[1] - pad[1]].cpu().numpy()
    e_m, e_d = float(np.abs(written - d[True]).mean()), float(np.abs(written - d[False]).mean())
    print(f"cli --mixed_precision: |written - mixed| {e_m:.2e}, |written - default| {e_d:.2e}")
    assert e_m < 1e-5
    assert e_d > 10 * max(e_m, 1e-7)

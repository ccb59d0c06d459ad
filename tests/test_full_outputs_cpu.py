"""forward(test_mode=False) without a GPU: the two refusals (both raised before any device check), the
sa_mask_upsample declarations of the header and the bindings, and the shape of
tests/golden/full_outputs.npz."""
import json
import re

import numpy as np
import pytest
import torch

from fixtures_util import load_fixture, regenerate_inputs
from stereoanywhere_amd import _native
from stereoanywhere_amd.model import ScheduleOptions, StereoAnywhere

PUBLISHED = dict(use_truncate_vol=True, use_aggregate_mono_vol=True)


def _zeros():
    x = torch.zeros(1, 3, 64, 128)
    return x, x, x[:, :1], x[:, :1]


def test_volume_corruption_is_refused():
    """The reference's default volume_corruption_prob (0.33) draws its training augmentations
    whenever not test_mode; they are not built."""
    m = StereoAnywhere(dict(PUBLISHED))
    assert m.args.volume_corruption_prob == 0.33
    with torch.no_grad(), pytest.raises(NotImplementedError, match="volume_corruption_prob=0"):
        m(*_zeros(), iters=1, test_mode=False)
    m = StereoAnywhere(dict(PUBLISHED, volume_corruption_prob=0.33))
    with torch.no_grad(), pytest.raises(NotImplementedError, match="volume_corruption_prob=0"):
        m(*_zeros(), iters=1, test_mode=False)


def test_grad_mode_is_refused():
    """Grad mode on with trainable parameters, or an input that requires grad: the outputs would
    carry no gradient."""
    m = StereoAnywhere(dict(PUBLISHED, volume_corruption_prob=0))
    assert torch.is_grad_enabled() and any(p.requires_grad for p in m.parameters())
    with pytest.raises(NotImplementedError, match=r"no gradient.*torch\.no_grad\(\)"):
        m(*_zeros(), iters=1, test_mode=False)
    for p in m.parameters():
        p.requires_grad_(False)
    x = list(_zeros())
    x[2] = x[2].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"no gradient.*torch\.no_grad\(\)"):
        m(*x, iters=1, test_mode=False)


def test_without_grad_the_call_reaches_the_device_check():
    """Neither refusal applies: the forward goes on to the device check (GPU only), as test mode does."""
    m = StereoAnywhere(dict(PUBLISHED, volume_corruption_prob=0))
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU only"):
        m(*_zeros(), iters=1, test_mode=False)


def test_schedule_option_defaults_on():
    assert ScheduleOptions().fuse_mask_upsample is True


def test_mask_upsample_is_declared():
    """The header and the bindings' table both carry the new entry points; the ABI version stays."""
    text = open(_native.HEADER).read()
    for name in ("sa_mask_upsample", "sa_mask_upsample_redo_blocks"):
        assert re.search(rf"\b{name}\(", text), name
        assert name in _native.SIGNATURES
    res, args = _native.SIGNATURES["sa_mask_upsample"]
    assert res is _native.I and len(args) == 13
    decl = re.search(r"int sa_mask_upsample\(([^;]*)\);", text).group(1)
    assert len(decl.split(",")) == 13
    assert _native.ABI_VERSION == 9 and "#define SA_ABI_VERSION 9" in text


def test_fixture_layout():
    fix = load_fixture("full_outputs.npz")
    H, W, seed = (int(v) for v in fix["shape"])
    assert (H, W, seed, float(fix["D"])) == (64, 128, 1, 24.0)
    regenerate_inputs(fix, 1, H, W, float(fix["D"]), seed0=seed)      # inputs_sha256
    tiny = load_fixture("tiny_64x128_it4.npz")
    assert str(fix["inputs_sha256"]) == str(tiny["inputs_sha256"])   # the input of tiny_64x128_it4.npz
    iters = int(fix["iters"])
    assert iters == 4
    cases = json.loads(str(fix["cases"]))
    assert cases == ["published", "agg_stereo", "vd1", "gru1_L2r3"]
    assert json.loads(str(fix["gru1_L2r3.args"])) == dict(n_gru_layers=1, corr_levels=2, corr_radius=3)
    for name in cases:
        f = fix[f"{name}.flow_predictions"]
        assert f.shape == (iters, 1, 1, H, W) and f.dtype == np.float32 and np.isfinite(f).all()
        maps = ["coarse_dispmono", "coarse_scaled_mde", "coarse_ldispmonoconf"]
        if json.loads(str(fix[f"{name}.args"])).get("use_aggregate_stereo_vol"):
            maps.append("coarse_dispstereo")
        else:
            assert f"{name}.coarse_dispstereo2" not in fix
        for key in maps:
            for view in "23":
                v = fix[f"{name}.{key}{view}"]
                assert v.shape == (1, 1, H, W) and v.dtype == np.float32 and np.isfinite(v).all()

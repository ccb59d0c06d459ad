"""Parameter names and shapes at every model geometry of tests/golden/geometry.npz equal the
reference's recorded ones (a checkpoint trained with a shallower GRU stack or a smaller lookup
loads with strict=True), and what stays unbuilt is refused at construction."""
import json
import os

import pytest
import torch

from fixtures_util import GOLDEN, load_fixture
from stereoanywhere_amd.model import StereoAnywhere

PUBLISHED = dict(use_truncate_vol=True, use_aggregate_mono_vol=True, vol_n_masks=8, n_additional_hourglass=0,
                 vol_downsample=0, mirror_conf_th=0.98, mirror_attenuation=0.9, lrc_th=1.0, normal_gain=10)


@pytest.fixture(scope="module")
def fix():
    return load_fixture("geometry.npz")


def _shapes(over):
    with torch.device("meta"):   # names and shapes only: no parameter is initialised
        return {k: list(v.shape) for k, v in StereoAnywhere(dict(PUBLISHED, **over)).state_dict().items()}


def _case_names(fix):
    return json.loads(str(fix["cases"])) + json.loads(str(fix["wide.cases"]))


def test_fixture_holds_the_table(fix):
    assert _case_names(fix) == ["gru2", "gru1", "L2", "L1r1", "L3r2", "r8", "gru2_L2r3", "gru1_L4r6", "nd3",
                                "base_96x160", "gru2_L3r5_96x160"]
    for name in _case_names(fix):
        assert (f"{name}.disparity" in fix) != (f"{name}.error" in fix)
    assert str(fix["nd3.error"]) == "IndexError"
    assert os.path.getsize(os.path.join(GOLDEN, "geometry.npz")) < 512 * 1024


def test_state_dict_matches_reference_at_every_geometry(fix):
    for name in _case_names(fix):
        over = json.loads(str(fix[f"{name}.args"]))
        ref = json.loads(str(fix[f"{name}.keys"]))
        got = _shapes(over)
        assert got == ref, (name, sorted(set(got) ^ set(ref)), [k for k in got if k in ref and got[k] != ref[k]])


def test_published_key_set_unchanged(fix):
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as f:
        ref = json.load(f)
    assert _shapes({}) == ref
    assert json.loads(str(fix["base_96x160.keys"])) == ref


def test_unbuilt_geometries_are_refused_at_construction():
    for over, msg in ((dict(corr_levels=5), "1..4 pyramid levels"), (dict(n_downsample=1), "n_downsample=2"),
                      (dict(corr_radius=9), "radius 1..8"), (dict(n_gru_layers=4), "GRU levels")):
        with pytest.raises(NotImplementedError, match=msg):
            StereoAnywhere(dict(PUBLISHED, **over))

"""The volume stage's own restatement (tests/volume_stage_ref.py) and draw_volume_corruption against
what the reference computed and drew (tests/golden/volume_stage.npz, volume_corruption_draws.json,
written by tests/golden/make_golden_volume_stage.py), and the measurement of the one tolerance the
GPU tests use.  No GPU."""
import json
import os
import random

import pytest
import torch

import volume_stage_ref as R
from fixtures_util import GOLDEN, load_fixture
from stereoanywhere_amd.diffops import VolumeCorruption, draw_volume_corruption

N_MASKS = 4


@pytest.fixture(scope="module")
def fix():
    return load_fixture("volume_stage.npz")


def golden_case(fix, name):
    """(plan, target's input volume, kwargs of R.stage for the target volume, reference outputs)."""
    t = {k: torch.from_numpy(fix[k]) for k in ("stereo_in", "mono_in", "mde2_lowres", "trunc_disp", "trunc_conf")}
    plan = json.loads(str(fix[f"{name}.plan"]))
    plan = None if plan is None else VolumeCorruption(*plan)
    trunc = (t["trunc_disp"], t["trunc_conf"], float(fix["trunc_atten"]))
    kw = {}
    if plan is not None:
        kw = dict(kind=plan.kind, mde=t["mde2_lowres"], nbins=N_MASKS, bin=plan.bin, shift=max(plan.shift, 1))
        if plan.kind == "noise":
            kw["noise"] = torch.from_numpy(fix[f"{name}.noise"])
    outs = {k: torch.from_numpy(fix[f"{name}.{k}"]) for k in ("stereo_out", "mono_out")}
    return plan, t, trunc, kw, outs


def own_outputs(plan, t, trunc, kw, dtype):
    s_kw = kw if plan is not None and plan.target == "stereo" else {}
    m_kw = kw if plan is not None and plan.target == "mono" else {}
    return (R.stage(t["stereo_in"], trunc=trunc, dtype=dtype, **s_kw), R.stage(t["mono_in"], dtype=dtype, **m_kw))


def test_golden_has_every_branch(fix):
    names = json.loads(str(fix["cases"]))
    assert names == ["none"] + [f"{t}_{k}" for t in ("stereo", "mono") for k in ("roll", "noise", "zero")]
    assert fix["stereo_in"].shape == fix["mono_in"].shape == (1, 1, 16, 32, 32)
    assert os.path.getsize(os.path.join(GOLDEN, "volume_stage.npz")) < 1 << 20
    for name in names[1:]:   # each case's mask selects something, and not everything
        plan = VolumeCorruption(*json.loads(str(fix[f"{name}.plan"])))
        m = R.bin_mask(torch.from_numpy(fix["mde2_lowres"]), N_MASKS, plan.bin)
        assert 0 < int(m.sum()) < m.numel(), name


def test_truncation_factor_is_the_references(fix):
    own = R.trunc_factor(torch.from_numpy(fix["trunc_disp"]), torch.from_numpy(fix["trunc_conf"]),
                         float(fix["trunc_atten"]), 32)
    assert torch.equal(own, torch.from_numpy(fix["trunc_out"]))


@pytest.mark.parametrize("name", ["none", "stereo_roll", "stereo_noise", "mono_roll", "mono_noise"])
def test_own_fp32_equals_reference_exactly(fix, name):
    plan, t, trunc, kw, outs = golden_case(fix, name)
    stereo, mono = own_outputs(plan, t, trunc, kw, torch.float32)
    assert torch.equal(stereo, outs["stereo_out"])
    assert torch.equal(mono, outs["mono_out"])


@pytest.mark.parametrize("name", ["stereo_zero", "mono_zero"])
def test_own_fp32_equals_reference_zero(fix, name):
    """The reference adds v*0 to the zeroed cell (its blend); the selected value is the same number."""
    plan, t, trunc, kw, outs = golden_case(fix, name)
    stereo, mono = own_outputs(plan, t, trunc, kw, torch.float32)
    assert torch.equal(stereo, outs["stereo_out"])
    assert torch.equal(mono, outs["mono_out"])


def test_blend_equals_selection():
    """For finite volumes and masks in {0, 1} the reference's blend v (1 - m) + src m is the selected
    value: roll and noise, every bin, shifts 1, W - 1 and W."""
    c = R.random_case(0, 2, 3, 37, 37)
    v = c["volume"]
    for b in range(N_MASKS):
        m = R.bin_mask(c["mde"], N_MASKS, b).half()   # generate_masks' dtype
        for shift in (1, 36, 37):
            blend = v * (1 - m) + torch.roll(v, shifts=shift, dims=3) * m
            assert torch.equal(blend, R.stage(v, "roll", c["mde"], N_MASKS, b, shift))
        blend = v * (1 - m) + v * c["noise"] * m
        assert torch.equal(blend, R.stage(v, "noise", c["mde"], N_MASKS, b, noise=c["noise"]))


def test_mask_edges():
    mde = torch.tensor([0.0, 0.25, 0.5, 1.0, -0.3, 0.2499999, 0.99999, float("nan")]).view(1, 1, 1, 8)
    got = [[int(x) for x in R.bin_mask(mde, 4, b).flatten()] for b in range(4)]
    assert got == [[1, 0, 0, 0, 0, 1, 0, 0], [0, 1, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0, 0],
                   [0, 0, 0, 0, 0, 0, 1, 0]]


def _replay(calls):
    """A stand-in rng that checks each call against the recorded one and returns its result."""
    class Replay:
        def __init__(self):
            self.i = 0

        def _next(self, name, args):
            assert self.i < len(calls), f"an extra call {name}{tuple(args)}"
            rec = calls[self.i]
            assert rec[:2] == [name, list(args)], f"call {self.i}: {name}{tuple(args)} where the reference made {rec[:2]}"
            self.i += 1
            return rec[2]

        def random(self):
            return self._next("random", [])

        def randint(self, a, b):
            return self._next("randint", [a, b])
    return Replay()


def _plan_of(calls):
    fired = [i for i, c in enumerate(calls) if c[0] == "random"]
    ints = [c[2] for c in calls if c[0] == "randint"]
    if not ints:
        return None
    target, kind = [(t, k) for t in ("stereo", "mono") for k in ("roll", "noise", "zero")][len(fired) - 1]
    return VolumeCorruption(target, kind, ints[0], ints[1] if kind == "roll" else 0)


def test_draws_match_the_reference():
    with open(os.path.join(GOLDEN, "volume_corruption_draws.json")) as f:
        d = json.load(f)
    assert sorted(map(int, d["seeds"])) == list(range(64))
    args = (d["prob"], d["n_masks"], d["w_lowres"])
    assert args == (0.33, 4, 32)
    seen = set()
    for seed, calls in d["seeds"].items():
        rng = _replay(calls)
        plan = draw_volume_corruption(*args, rng=rng)
        assert rng.i == len(calls), f"seed {seed}: {len(calls) - rng.i} recorded calls were not made"
        assert plan == _plan_of(calls), seed
        # and a seeded random.Random gives the recorded values
        assert draw_volume_corruption(*args, rng=random.Random(int(seed))) == plan
        seen.add(None if plan is None else plan[:2])
    assert len(seen) >= 6   # "none" and at least five of the six branches occur among the seeds
    for other in d["other"]:
        rng = _replay(other["calls"])
        plan = draw_volume_corruption(other["prob"], args[1], args[2], rng=rng)
        assert rng.i == len(other["calls"])
        if other["prob"] == 0:
            assert plan is None and [c[0] for c in other["calls"]] == ["random"] * 6
        else:
            assert plan is not None and plan[:2] == ("stereo", "roll") and len(other["calls"]) == 3


def test_draw_uses_the_module_by_default():
    random.seed(5)
    a = draw_volume_corruption(0.33, 4, 32)
    assert a == draw_volume_corruption(0.33, 4, 32, rng=random.Random(5))


def test_measured_tolerance(fix):
    """E of volume_stage_ref: the largest relative deviation of fp32 results (the reference's captured
    ones, and the fp32 restatement on the random cases) from the float64 restatement."""
    worst = {}

    def take(what, x32, ref64):
        worst[what] = max(worst.get(what, 0.0), R.rel_deviation(x32, ref64))

    disp, conf = torch.from_numpy(fix["trunc_disp"]), torch.from_numpy(fix["trunc_conf"])
    atten = float(fix["trunc_atten"])
    take("factor", torch.from_numpy(fix["trunc_out"]), R.trunc_factor(disp, conf, atten, 32, torch.float64))
    for name, what, key in (("none", "truncated", "stereo_out"), ("stereo_zero", "zero+truncated", "stereo_out"),
                            ("mono_zero", "zero", "mono_out")):
        plan, t, trunc, kw, outs = golden_case(fix, name)
        stereo, mono = own_outputs(plan, t, trunc, kw, torch.float64)
        take(what, outs[key], stereo if key == "stereo_out" else mono)
    for seed in range(4):
        c = R.random_case(seed, 2, 3, 37, 37)
        for atten in (0.9, 0.1):
            take("factor", R.trunc_factor(c["disp"], c["conf"], atten, 37), R.trunc_factor(c["disp"], c["conf"], atten, 37, torch.float64))
            trunc = (c["disp"], c["conf"], atten)
            take("truncated", R.stage(c["volume"], trunc=trunc), R.stage(c["volume"], trunc=trunc, dtype=torch.float64))
            for b in (0, 3):
                kw = dict(kind="zero", mde=c["mde"], nbins=4, bin=b)
                take("zero", R.stage(c["volume"], **kw), R.stage(c["volume"], dtype=torch.float64, **kw))
                take("zero+truncated", R.stage(c["volume"], trunc=trunc, **kw),
                     R.stage(c["volume"], trunc=trunc, dtype=torch.float64, **kw))
    print({k: f"{v:.3e}" for k, v in worst.items()}, "E", R.E)
    assert max(worst.values()) <= R.E
    assert max(worst.values()) >= R.E / 2   # the constant is the measurement, not a generous bound

"""Generate tests/golden/volume_stage.npz and tests/golden/volume_corruption_draws.json by running
the REFERENCE's forward(test_mode=False) with its volume-corruption augmentations on
(volume_corruption_prob = 0.33, stereoanywhere.py:214-255).

Test infrastructure only, run where the reference is mounted (see make_golden.py):

    python tests/golden/make_golden_volume_stage.py

volume_stage.npz: the 64x128 input of tiny_64x128_it4.npz (volumes [1,1,16,32,32]), seeded weights,
one iteration.  One seed per augmentation branch and one where none fires (found with
stereoanywhere_amd.diffops.draw_volume_corruption); per case the plan, the noise the reference drew
and the two volumes it handed to corr_block(...).  The inputs of the stage are the same in every case
and are stored once: both pre-stage volumes, mde2_lowres, truncate_corr_volume_v2's arguments and
result.  Byte-identical captures are stored once (make_golden._dedupe).

volume_corruption_draws.json: for seeds 0..63 at (0.33, 4, 32), plus prob 0 and 1, the sequence of
calls the reference makes on its `random` module and their results.
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import _dedupe, _load_reference, _np, _pair_record, _single_thread_lsq, build_model  # noqa: E402
from stereoanywhere_amd import synth  # noqa: E402
from stereoanywhere_amd.diffops import _BRANCHES, draw_volume_corruption  # noqa: E402

TINY = (64, 128, 24.0, 1)   # H, W, max disparity, seed: the input of tiny_64x128_it4.npz
PROB, N_MASKS, W_LOWRES = 0.33, 4, 32
DRAW_SEEDS = range(64)


class RecordingRandom:
    """Stand-in for the reference module's `random`: a seeded random.Random whose calls are listed."""

    def __init__(self, seed):
        self._rng = random.Random(seed)
        self.calls = []

    def random(self):
        v = self._rng.random()
        self.calls.append(["random", [], v])
        return v

    def randint(self, a, b):
        v = self._rng.randint(a, b)
        self.calls.append(["randint", [a, b], v])
        return v


def run_stage(sa_mod, corr_mod, model, t, seed, prob):
    """One reference forward(test_mode=False, iters=1) -> (captures, the calls on `random`)."""
    cap = {"corr": [], "blocks": [], "rand_like": []}
    rng = RecordingRandom(seed)
    saved = dict(random=sa_mod.random, generate_masks=sa_mod.generate_masks,
                 trunc=sa_mod.truncate_corr_volume_v2, corr=corr_mod.CorrBlock1D.corr,
                 init=corr_mod.CorrBlock1D.__init__, rand_like=torch.rand_like)

    def masks(mde, N=16):
        if N == model.args.vol_aug_n_masks and "mde2_lowres" not in cap and len(cap["corr"]) == 2:
            cap["mde2_lowres"] = _np(mde)
        return saved["generate_masks"](mde, N=N)

    def trunc(disp, conf, **kw):
        out = saved["trunc"](disp, conf, **kw)
        cap.update(trunc_disp=_np(disp), trunc_conf=_np(conf), trunc_out=_np(out),
                   trunc_atten=np.array(kw["attenuation_gain"], np.float64))
        assert kw["conf_th"] is None
        return out

    def corr(f2, f3):
        out = saved["corr"](f2, f3)
        cap["corr"].append(_np(out))
        return out

    def init(self, fullcorr, *a, **k):
        cap["blocks"].append(_np(fullcorr))
        saved["init"](self, fullcorr, *a, **k)

    def rand_like(x, *a, **k):
        out = saved["rand_like"](x, *a, **k)
        cap["rand_like"].append((str(out.dtype), _np(out)))
        return out

    hook = model.classifier_mono.register_forward_hook(lambda mod, inp, out: cap.__setitem__("mono_in", _np(out)))
    restore = _single_thread_lsq(sa_mod)
    sa_mod.random, sa_mod.generate_masks, sa_mod.truncate_corr_volume_v2 = rng, masks, trunc
    corr_mod.CorrBlock1D.corr = staticmethod(corr)
    corr_mod.CorrBlock1D.__init__ = init
    torch.rand_like = rand_like
    model.args.volume_corruption_prob = prob
    try:
        torch.manual_seed(seed)
        with torch.no_grad():
            model(*t, iters=1, test_mode=False)
    finally:
        sa_mod.random, sa_mod.generate_masks = saved["random"], saved["generate_masks"]
        sa_mod.truncate_corr_volume_v2 = saved["trunc"]
        corr_mod.CorrBlock1D.corr = staticmethod(saved["corr"])
        corr_mod.CorrBlock1D.__init__ = saved["init"]
        torch.rand_like = saved["rand_like"]
        restore()
        hook.remove()
    return cap, rng.calls


def _volume(fullcorr):
    """[B,H,W1,1,W2] as handed to corr_block -> [B,1,H,W1,W2]."""
    return np.ascontiguousarray(fullcorr[:, :, :, 0, :][:, None])


def main():
    torch.set_num_threads(8)
    sa_mod, _, corr_mod = _load_reference()
    model = build_model(sa_mod)
    assert model.args.volume_corruption_prob == PROB and model.args.vol_aug_n_masks == N_MASKS
    assert model.args.use_truncate_vol and model.args.use_aggregate_mono_vol and not model.args.use_aggregate_stereo_vol
    H, W, D, seed = TINY
    pair = synth.synthetic_batch(1, H, W, D, seed0=seed)
    t = [torch.from_numpy(pair[k]) for k in ("left", "right", "mono_left", "mono_right")]

    # the draws of every seed, and the plan draw_volume_corruption makes of them
    draws = {"prob": PROB, "n_masks": N_MASKS, "w_lowres": W_LOWRES, "seeds": {}, "other": []}
    plans = {}
    for s in DRAW_SEEDS:
        _, calls = run_stage(sa_mod, corr_mod, model, t, s, PROB)
        draws["seeds"][str(s)] = calls
        plans[s] = draw_volume_corruption(PROB, N_MASKS, W_LOWRES, random.Random(s))
        print("seed", s, plans[s], len(calls), "calls", flush=True)
    for p in (0.0, 1.0):
        _, calls = run_stage(sa_mod, corr_mod, model, t, 0, p)
        draws["other"].append({"prob": p, "seed": 0, "calls": calls})
    with open(os.path.join(HERE, "volume_corruption_draws.json"), "w") as f:
        json.dump(draws, f, indent=0)

    # one seed per branch, one where none fires: the smallest of each (the last branch fires for
    # 4 % of the seeds and for none of the first 64)
    wanted = [None] + list(_BRANCHES)
    chosen = {}
    for s in range(1000):
        plans[s] = draw_volume_corruption(PROB, N_MASKS, W_LOWRES, random.Random(s))
        key = None if plans[s] is None else (plans[s].target, plans[s].kind)
        chosen.setdefault(key, s)
    assert all(k in chosen for k in wanted), sorted(map(str, chosen))

    out = {"shape": np.array([H, W, seed], np.int64), "D": np.array(D), **_pair_record(pair)}
    names = []
    torch.set_num_threads(1)   # the stage's inputs must be the same bytes in every case
    for key in wanted:
        s = chosen[key]
        name = "none" if key is None else f"{key[0]}_{key[1]}"
        names.append(name)
        cap, calls = run_stage(sa_mod, corr_mod, model, t, s, PROB)
        plan = plans[s]
        stereo_in = _volume(cap["corr"][0])
        assert len(cap["corr"]) == 2 and len(cap["blocks"]) == 2
        inputs = dict(stereo_in=stereo_in, mono_in=cap["mono_in"], mde2_lowres=cap["mde2_lowres"],
                      trunc_disp=cap["trunc_disp"], trunc_conf=cap["trunc_conf"], trunc_out=cap["trunc_out"],
                      trunc_atten=cap["trunc_atten"])
        for k, v in inputs.items():   # the same in every case: stored once
            if k in out:
                assert np.array_equal(out[k], v), (name, k, float(np.abs(out[k] - v).max()))
            out[k] = v
        out[f"{name}.seed"] = np.array(s)
        out[f"{name}.plan"] = np.array(json.dumps(None if plan is None else list(plan)))
        out[f"{name}.stereo_out"] = _volume(cap["blocks"][0])
        out[f"{name}.mono_out"] = _volume(cap["blocks"][1])
        if plan is not None and plan.kind == "noise":
            (dtype, noise), = cap["rand_like"]
            assert dtype == "torch.float16" and noise.shape == (1, 1, H // 4, W // 4, 1), (dtype, noise.shape)
            out[f"{name}.noise"] = noise.astype(np.float16)   # _np widened it: the values are fp16
        else:
            assert not cap["rand_like"]
        print(name, "seed", s, plan, [c[:2] for c in calls], flush=True)
    out["cases"] = np.array(json.dumps(names))
    for k, v in out.items():
        if isinstance(v, np.ndarray) and v.dtype.kind == "f":
            assert np.isfinite(v).all(), k
    path = os.path.join(HERE, "volume_stage.npz")
    np.savez_compressed(path, **_dedupe(out))
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()

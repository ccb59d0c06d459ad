"""Generate tests/golden/full_outputs.npz by running the REFERENCE's default call form,
forward(test_mode=False) (stereoanywhere.py:95, 299), with volume_corruption_prob=0 (no training
augmentation drawn) under torch.no_grad().

Test infrastructure only, run where the reference is mounted (see make_golden.py):

    python tests/golden/make_golden_full_outputs.py

Per case: the per-iteration up-sampled predictions and every non-None coarse map of the returned
tuple.  Seeded weights (seed 0), 4 iterations, the 64x128 input of tiny_64x128_it4.npz, the
single-threaded least-squares solve the other fixtures pin.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF_ARGS, _dedupe, _load_reference, _np, _pair_record, _single_thread_lsq  # noqa: E402
from stereoanywhere_amd import synth  # noqa: E402

ITERS = 4
TINY = (64, 128, 24.0, 1)   # H, W, max disparity, seed: the input of tiny_64x128_it4.npz
CASES = [
    ("published", dict()),
    ("agg_stereo", dict(use_aggregate_stereo_vol=True)),
    ("vd1", dict(vol_downsample=1)),
    ("gru1_L2r3", dict(n_gru_layers=1, corr_levels=2, corr_radius=3)),   # the fold lookup
]
# positions of the returned tuple's two coarse lists and two confidence lists
COARSE = ("dispstereo", "dispmono", "scaled_mde")


def full_outputs_cases(sa_mod):
    H, W, D, seed = TINY
    pair = synth.synthetic_batch(1, H, W, D, seed0=seed)
    out = {"iters": np.array(ITERS), "shape": np.array([H, W, seed], np.int64), "D": np.array(D),
           "cases": np.array(json.dumps([n for n, _ in CASES])), **_pair_record(pair)}
    t = [torch.from_numpy(pair[k]) for k in ("left", "right", "mono_left", "mono_right")]
    restore = _single_thread_lsq(sa_mod)
    try:
        for name, over in CASES:
            torch.manual_seed(0)
            model = sa_mod.StereoAnywhere(dict(REF_ARGS, volume_corruption_prob=0, **over)).eval()
            synth.load_seeded_weights(model, seed=0)
            with torch.no_grad():
                flows, confs, c2, c3, l2, l3 = model(*t, iters=ITERS, test_mode=False)
            assert len(flows) == ITERS and confs == [None] * ITERS
            assert l2[0] is None and l2[2] is None and l3[0] is None and l3[2] is None
            out[f"{name}.args"] = np.array(json.dumps(over, sort_keys=True))
            out[f"{name}.flow_predictions"] = np.stack([_np(f) for f in flows]).astype(np.float32)
            for view, coarse, conf in (("2", c2, l2), ("3", c3, l3)):
                for key, v in zip(COARSE, coarse):
                    if v is not None:
                        out[f"{name}.coarse_{key}{view}"] = _np(v).astype(np.float32)
                out[f"{name}.coarse_ldispmonoconf{view}"] = _np(conf[1]).astype(np.float32)
            stored = sorted(k for k in out if k.startswith(name + ".coarse_"))
            print(name, "flow range", float(out[f"{name}.flow_predictions"].min()),
                  float(out[f"{name}.flow_predictions"].max()), [k.split(".")[1] for k in stored], flush=True)
            for k in stored:
                assert np.isfinite(out[k]).all(), k
                print("  ", k, tuple(out[k].shape), float(out[k].min()), float(out[k].max()), flush=True)
    finally:
        restore()
    return out


def main():
    torch.set_num_threads(8)
    sa_mod, _, _ = _load_reference()
    # (cases that share the mono branch return byte-identical coarse mono maps: stored once, read
    # back through fixtures_util.load_fixture's aliases)
    np.savez_compressed(os.path.join(HERE, "full_outputs.npz"), **_dedupe(full_outputs_cases(sa_mod)))


if __name__ == "__main__":
    main()

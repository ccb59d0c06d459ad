"""Generate tests/golden/geometry.npz by running the REFERENCE under non-published model
geometries (n_gru_layers, corr_levels, corr_radius; stereoanywhere.py:26-29).

Test infrastructure only, run where the reference is mounted (see make_golden.py):

    python tests/golden/make_golden_geometry.py

Per case: the reference's state-dict names and shapes (JSON) and its final disparity, or the
exception type where the reference itself fails.  Seeded weights (seed 0), 4 iterations, the
single-threaded least-squares solve the other fixtures pin (run_capture).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF_ARGS, _load_reference, _pair_record, run_capture  # noqa: E402
from stereoanywhere_amd import synth  # noqa: E402

ITERS = 4
# every case below runs on the input of tiny_64x128_it4.npz (64x128, D = 24, seed 1), whose mono
# branch and least-squares solve are pinned as stable; it is recorded once (inputs_sha256)
TINY = (64, 128, 24.0, 1)
GEOMETRY_CASES = [
    ("gru2", dict(n_gru_layers=2)),
    ("gru1", dict(n_gru_layers=1)),
    ("L2", dict(corr_levels=2)),
    ("L1r1", dict(corr_levels=1, corr_radius=1)),
    ("L3r2", dict(corr_levels=3, corr_radius=2)),
    ("r8", dict(corr_radius=8)),
    ("gru2_L2r3", dict(n_gru_layers=2, corr_levels=2, corr_radius=3)),
    ("gru1_L4r6", dict(n_gru_layers=1, corr_radius=6)),
    ("nd3", dict(n_downsample=3)),   # the reference raises IndexError in its own forward
]
# 96x160: W/4 = 40 (level widths 40, 20, 10, 5) and W/16 = 10, a ragged GRU plane.  This input is
# not pinned as well-conditioned for the reference's quantile-band least squares (the note at
# make_golden.FLAG_CASES), so the published geometry runs on it too (base_96x160): the GPU
# test checks that pair first.  Seed 1 held (see tests/test_gpu_model_geometry.py); a seed
# whose base pair misses 1e-3 is replaced by the next one here.
WIDE = (96, 160, 32.0, 1)
WIDE_CASES = [
    ("base_96x160", dict()),
    ("gru2_L3r5_96x160", dict(n_gru_layers=2, corr_levels=3, corr_radius=5)),
]


def _run(sa_mod, ut, corr_mod, name, over, pair, out):
    torch.manual_seed(0)
    model = sa_mod.StereoAnywhere(dict(REF_ARGS, **over)).eval()
    synth.load_seeded_weights(model, seed=0)
    out[f"{name}.args"] = np.array(json.dumps(over, sort_keys=True))
    out[f"{name}.keys"] = np.array(json.dumps({k: list(v.shape) for k, v in model.state_dict().items()},
                                              sort_keys=True))
    try:
        d = run_capture(sa_mod, ut, corr_mod, model, pair, ITERS, capture_all=False)["disparity"]
        out[f"{name}.disparity"] = d.astype(np.float32)
        print(name, "disp range", float(d.min()), float(d.max()), flush=True)
    except Exception as e:  # the reference's own failure on this geometry
        out[f"{name}.error"] = np.array(type(e).__name__)
        print(name, "raises", type(e).__name__, str(e)[:120], flush=True)


def geometry_cases(sa_mod, ut, corr_mod):
    out = {"iters": np.array(ITERS)}
    for prefix, shape, cases in (("", TINY, GEOMETRY_CASES), ("wide.", WIDE, WIDE_CASES)):
        H, W, D, seed = shape
        pair = synth.synthetic_batch(1, H, W, D, seed0=seed)
        out.update(_pair_record(pair, prefix))
        out[prefix + "shape"] = np.array([H, W, seed], np.int64)
        out[prefix + "D"] = np.array(D)
        out[prefix + "cases"] = np.array(json.dumps([n for n, _ in cases]))
        for name, over in cases:
            _run(sa_mod, ut, corr_mod, name, over, pair, out)
    return out


def main():
    torch.set_num_threads(8)
    sa_mod, ut, corr_mod = _load_reference()
    np.savez_compressed(os.path.join(HERE, "geometry.npz"), **geometry_cases(sa_mod, ut, corr_mod))


if __name__ == "__main__":
    main()

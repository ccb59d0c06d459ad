"""Generate tests/golden/mixed.npz: the REFERENCE in fp32 and under its own mixed precision
(torch.autocast, float16, as test.py:189, 215 wrap the forward; on the CPU here), published geometry.

Test infrastructure only, run where the reference is mounted (see make_golden.py):

    python tests/golden/make_golden_mixed.py

Per case: the input digest, the reference's fp32 disparity, its f16-autocast disparity and the EPE
between the two, which is the accuracy contract of this build's mixed-precision mode
(tests/test_gpu_model_mixed.py: no further from the reference's fp32 output than the reference's
own mixed precision is).  Seeded weights (seed 0), synthetic inputs of seed 0, the single-threaded
least-squares solve the other fixtures pin (run_capture).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import _load_reference, _pair_record, build_model, run_capture  # noqa: E402
from stereoanywhere_amd import synth  # noqa: E402

# (name, H, W, max disparity, iterations, input seed); 96x160: W/16 = 10, a ragged GRU plane
MIXED_CASES = [
    ("tiny", 64, 128, 16.0, 4, 0),
    ("wide", 96, 160, 24.0, 8, 0),
]


def mixed_cases(sa_mod, ut, corr_mod):
    model = build_model(sa_mod)
    out = {"cases": np.array(",".join(c[0] for c in MIXED_CASES))}
    for name, H, W, D, iters, seed in MIXED_CASES:
        pair = synth.synthetic_batch(1, H, W, D, seed0=seed)
        out.update(_pair_record(pair, name + "."))
        out[name + ".shape"] = np.array([H, W, seed, iters], np.int64)
        out[name + ".D"] = np.array(D)
        d32 = run_capture(sa_mod, ut, corr_mod, model, pair, iters, capture_all=False)["disparity"]
        with torch.autocast("cpu", dtype=torch.float16):
            d16 = run_capture(sa_mod, ut, corr_mod, model, pair, iters, capture_all=False)["disparity"]
        d32, d16 = d32.astype(np.float32), d16.astype(np.float32)
        assert np.isfinite(d32).all() and np.isfinite(d16).all()
        diff = np.abs(d16.astype(np.float64) - d32)
        out[name + ".disparity"] = d32
        out[name + ".disparity_autocast_f16"] = d16
        out[name + ".epe_autocast_f16"] = np.array(diff.mean())
        print(name, "disp range", float(d32.min()), float(d32.max()), "autocast EPE", float(diff.mean()),
              "max", float(diff.max()), flush=True)
    return out


def main():
    torch.set_num_threads(8)
    sa_mod, ut, corr_mod = _load_reference()
    np.savez_compressed(os.path.join(HERE, "mixed.npz"), **mixed_cases(sa_mod, ut, corr_mod))


if __name__ == "__main__":
    main()

"""Numerics of the mixed-precision F(4x4) scheme (tests/mixed_ref.py: the Winograd-domain input as
a single f16, exact filter pairs, fp32 sums) against an fp64 direct conv, on the CPU.  It is a real
rounding (far above the split scheme's error) and stays within a small factor of what f16 autocast
gives a direct conv (x and w rounded to f16): F(4x4)'s input transform amplifies values up to
100-fold before the rounding, which is where the factor comes from."""
import numpy as np
import pytest

from mixed_ref import direct_f16_operands, wino4_mixed
from test_split_numerics_cpu import direct, wino4


def _rel(y, ref):
    return float(np.abs(y - ref).mean() / np.abs(ref).mean())


@pytest.mark.parametrize("seed,relu_like", [(0, False), (1, False), (2, True)])
def test_mixed_scheme_error_bounds(seed, relu_like):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((128, 32, 32)).astype(np.float32)
    if relu_like:
        x = np.maximum(x, 0.0)
    w = (rng.standard_normal((32, 128, 3, 3)) / (3 * 128 ** 0.5)).astype(np.float32)
    ref = direct(x, w)
    e_mixed = _rel(wino4_mixed(x, w), ref)
    e_split = _rel(wino4(x, w, True), ref)
    e_f16 = _rel(direct_f16_operands(x, w), ref)
    print(f"seed {seed} relu_like {relu_like}: mixed {e_mixed:.3e}, split {e_split:.3e}, f16 operands {e_f16:.3e} "
          f"(mixed / f16 {e_mixed / e_f16:.2f})")
    assert e_mixed >= 20 * e_split, (e_mixed, e_split)     # a real rounding, not the split scheme
    assert e_mixed <= 8 * e_f16, (e_mixed, e_f16)          # measured 4.8-6.0x


def test_mixed_restatement_pads_ragged_rows():
    """H not a multiple of 4: the restatement zero-pads the rows, as the kernel's tiles do."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((8, 9, 12)).astype(np.float32)
    w = (rng.standard_normal((32, 8, 3, 3)) / 8).astype(np.float32)
    y, ref = wino4_mixed(x, w), direct(x, w)
    assert y.shape == ref.shape
    assert _rel(y, ref) < 1e-2

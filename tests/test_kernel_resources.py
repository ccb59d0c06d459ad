"""Compile-time checks of the hot kernels (hipcc for gfx950, no GPU): no register spills (scratch)
in the conv kernels whose second, rarely taken passes (the split kernels' range guards) share a
body with the hot one, or whose register budget is near the limit (conv3d_s2mf: ~239 VGPRs)."""
import os

import pytest

from stereoanywhere_amd._native import resource_usage

HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.mark.parametrize("name,kernel", [
    ("conv2d_wino4.hip", "wino_f4k3_kernel"),
    ("conv3d_mfma.hip", "conv3d_mf_kernel"),
    ("conv3d_s2mf.hip", "conv3d_s2mf_kernel"),
])
def test_conv_kernels_do_not_spill(tmp_path, name, kernel):
    usage = resource_usage(name, tmp_path)
    hot = {k: u["scratch"] for k, u in usage.items() if kernel in k}
    print({k: usage[k] for k in hot})
    assert hot, sorted(usage)
    # the one measured exception: the split F(4x4) kernel with the affine input on the paired loop
    # spills a few loop-invariant values and is faster than without (A/B in
    # profiles/ab/r06_w4_pair_ab.txt); bounded, so a real regression still fails
    allowed = {k: 32 for k in hot if "W4CfgILi8ELi8ELb1EEELb0ELb1E" in k}
    assert all(v <= allowed.get(k, 0) for k, v in hot.items()), hot


def test_makefile_builds_wino4_without_slp_vectorize():
    """The product build of conv2d_wino4.hip must keep -fno-slp-vectorize (the no-spill build the
    check above compiles): without it the split instances spill and gave wrong results on the GPU."""
    mk = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "Makefile")).read()
    assert any(line.startswith("build/conv2d_wino4.o:") and "-fno-slp-vectorize" in line for line in mk.splitlines())

"""Compile-time check of the correlation plug-in's backward kernels (hipcc for gfx950, no GPU), read
from the compile's resource-usage remarks only: every kernel of corr_backward.hip runs without
scratch.  The printed VGPR / AGPR / LDS figures are the ones in DESIGN.md's resource table."""
import os

import pytest

from stereoanywhere_amd._native import resource_usage

HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

KERNELS = ["lookup_backward_kernelILb1E", "lookup_backward_kernelILb0E", "pyramid_backward_kernelILb1E",
           "pyramid_backward_kernelILb0E", "volume_backward_kernelILb1E", "volume_backward_kernelILb0E"]


def test_backward_kernels_do_not_spill(tmp_path):
    usage = resource_usage("corr_backward.hip", tmp_path)
    assert len(usage) == len(KERNELS), sorted(usage)
    for k in KERNELS:
        (name, u), = [(n, v) for n, v in usage.items() if k in n]
        print(f"{k}: VGPRs {u['vgprs']} AGPRs {u['agprs']} scratch {u['scratch']} LDS {u['lds']} "
              f"occupancy {u['occupancy']}")
        assert u["scratch"] == 0, name
        # the static LDS of a block stays under the 64 KiB a kernel may declare
        assert u["lds"] <= 64 * 1024, name

"""Compile-time check of the soft-argmin / convex up-sampling backward kernels (hipcc for gfx950, no
GPU), read from the compile's resource-usage remarks only: every kernel of diffops_backward.hip runs
without scratch.  The printed VGPR / LDS / occupancy figures are the ones in DESIGN.md section 4e."""
import os

import pytest

from stereoanywhere_amd._native import resource_usage

HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

KERNELS = ["sab_ystats_kernelILb1E", "sab_ystats_kernelILb0E", "sab_grad_kernel", "cub_mask_kernelILi4E",
           "cub_mask_kernelILi0E", "cub_flow_kernelILi4E", "cub_flow_kernelILi0E"]


def test_backward_kernels_do_not_spill(tmp_path):
    usage = resource_usage("diffops_backward.hip", tmp_path)
    assert len(usage) == len(KERNELS), sorted(usage)
    for k in KERNELS:
        (name, u), = [(n, v) for n, v in usage.items() if k in n]
        print(f"{k}: VGPRs {u['vgprs']} AGPRs {u['agprs']} scratch {u['scratch']} LDS {u['lds']} "
              f"occupancy {u['occupancy']}")
        assert u["scratch"] == 0, name
        assert u["lds"] <= 64 * 1024, name

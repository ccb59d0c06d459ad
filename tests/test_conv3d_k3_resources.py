"""Compile-time check of the 3x3x3 conv backward's kernels (hipcc for gfx950 at the Makefile's -O3, no GPU), read
from the compile's resource-usage remarks only: no kernel of conv3d_backward.hip uses scratch, each kernel's
VGPRs, LDS bytes and waves per SIMD are DESIGN.md section 4l's table, and the three instances of conv3d_mf_kernel
(conv3d_mfma.hip), whose epilogue gained a per-sample factor, keep the scratch, LDS and occupancy they had."""
import os

import pytest

from stereoanywhere_amd._native import resource_usage

HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# kernel -> (VGPRs, LDS bytes per block, waves per SIMD): DESIGN.md 4l
EXPECTED = {"sample_scale_kernel": (17, 16, 8), "bw_fold_kernel": (10, 0, 8),
            "bw_kernelILi8EE": (200, 55296, 2), "bw_kernelILi16EE": (200, 110592, 2),
            "bw_kernelILi32EE": (195, 122368, 2)}
# conv3d_mf_kernel<C, C> -> (LDS bytes per block, waves per SIMD, most VGPRs + AGPRs) before the factor
FORWARD = {8: (130112, 2, 237), 16: (117376, 2, 249), 32: (107776, 1, 366)}


def test_backward_kernels_match_the_table(tmp_path):
    usage = resource_usage("conv3d_backward.hip", tmp_path)
    assert len(usage) == len(EXPECTED), sorted(usage)
    for k, (vgprs, lds, occupancy) in EXPECTED.items():
        (name, u), = [(n, v) for n, v in usage.items() if k in n]
        print(f"{k}: VGPRs {u['vgprs']} AGPRs {u['agprs']} scratch {u['scratch']} LDS {u['lds']} "
              f"occupancy {u['occupancy']}")
        assert u["scratch"] == 0, name
        assert (u["vgprs"], u["lds"], u["occupancy"]) == (vgprs, lds, occupancy), name


def test_forward_kernels_keep_their_resources(tmp_path):
    usage = resource_usage("conv3d_mfma.hip", tmp_path)
    for c, (lds, occupancy, regs) in FORWARD.items():
        (name, u), = [(n, v) for n, v in usage.items() if f"conv3d_mf_kernelILi{c}ELi{c}EE" in n]
        print(f"conv3d_mf_kernel<{c}, {c}>: VGPRs {u['vgprs']} AGPRs {u['agprs']} scratch {u['scratch']} "
              f"LDS {u['lds']} occupancy {u['occupancy']}")
        assert u["scratch"] == 0, name
        assert (u["lds"], u["occupancy"]) == (lds, occupancy), name
        assert u["vgprs"] + u["agprs"] <= regs, name

"""Compile-time check of the fused training-loss kernels (hipcc for gfx950, no GPU), read from the
compile's resource-usage remarks only: no kernel of losses.hip uses scratch (the maps of a launch
are indexed in the kernel arguments, not in a private copy) and each stays within 64 KiB of LDS.  The
printed VGPR / LDS / occupancy figures are the ones in DESIGN.md section 4g."""
import os

import pytest

from stereoanywhere_amd._native import resource_usage

HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

KERNELS = ["loss_stats_kernel", "loss_fwd_kernel", "loss_finalise_kernel", "loss_bwd_kernel"]


def test_loss_kernels_do_not_spill(tmp_path):
    usage = resource_usage("losses.hip", tmp_path)
    assert len(usage) == len(KERNELS), sorted(usage)
    for k in KERNELS:
        (name, u), = [(n, v) for n, v in usage.items() if k in n]
        print(f"{k}: VGPRs {u['vgprs']} AGPRs {u['agprs']} scratch {u['scratch']} LDS {u['lds']} "
              f"occupancy {u['occupancy']}")
        assert u["scratch"] == 0, name
        assert u["lds"] <= 64 * 1024, name

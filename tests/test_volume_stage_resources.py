"""Compile-time check of the volume-stage kernels (hipcc for gfx950, no GPU), read from the compile's
resource-usage remarks only: no kernel of volume_stage.hip uses scratch, the streaming kernels use no
LDS and every kernel keeps the full 8 waves per SIMD.  The printed VGPR / LDS / occupancy figures are
the ones in DESIGN.md section 4h."""
import os

import pytest

from stereoanywhere_amd._native import resource_usage

HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# the eight (kind, truncation) instances of the stage, then the two steps of the maximum
STAGE = [f"volume_stage_kernelILi{kind}ELb{trunc}E" for kind in range(4) for trunc in (0, 1)]
PEAK = ["volume_peak_partial_kernel", "volume_peak_final_kernel"]


def test_volume_stage_kernels_do_not_spill(tmp_path):
    usage = resource_usage("volume_stage.hip", tmp_path)
    assert len(usage) == len(STAGE) + len(PEAK), sorted(usage)
    for k in STAGE + PEAK:
        (name, u), = [(n, v) for n, v in usage.items() if k in n]
        print(f"{k}: VGPRs {u['vgprs']} AGPRs {u['agprs']} scratch {u['scratch']} LDS {u['lds']} "
              f"occupancy {u['occupancy']}")
        assert u["scratch"] == 0, name
        assert u["occupancy"] == 8, name
        assert u["lds"] == (0 if k in STAGE else 32), name

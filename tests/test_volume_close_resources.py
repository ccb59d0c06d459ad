"""Compile-time check of the volume-close kernels (hipcc for gfx950, no GPU), read from the compile's
resource-usage remarks only: no kernel of volume_close.hip uses scratch and every kernel keeps the full
8 waves per SIMD.  The printed VGPR / LDS / occupancy figures are the ones in DESIGN.md section 4j."""
import os

import pytest

from stereoanywhere_amd._native import resource_usage

HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# the gate-less and gated instances of the two backward launches, the statistics pass and the fold
KERNELS = ["close_stats_kernel", "close_bwd_fold_kernel"] + [
    f"close_bwd_{step}_kernelILb{gated}E" for step in ("reduce", "apply") for gated in (0, 1)]
# bytes per block: two float64 sums per wave; the gated reduce adds a tile of dgl sums per wave
LDS = {"close_stats_kernel": 64, "close_bwd_fold_kernel": 0, "close_bwd_reduce_kernelILb0E": 64,
       "close_bwd_reduce_kernelILb1E": 64 + 4 * 256 * 4, "close_bwd_apply_kernelILb0E": 0,
       "close_bwd_apply_kernelILb1E": 0}


def test_volume_close_kernels_do_not_spill(tmp_path):
    usage = resource_usage("volume_close.hip", tmp_path)
    assert len(usage) == len(KERNELS), sorted(usage)
    for k in KERNELS:
        (name, u), = [(n, v) for n, v in usage.items() if k in n]
        print(f"{k}: VGPRs {u['vgprs']} AGPRs {u['agprs']} scratch {u['scratch']} LDS {u['lds']} "
              f"occupancy {u['occupancy']}")
        assert u["scratch"] == 0, name
        assert u["occupancy"] == 8, name
        assert u["lds"] == LDS[k], name

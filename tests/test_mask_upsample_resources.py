"""Compile-time check of sa_mask_upsample's kernels (hipcc for gfx950, no GPU), read from the compile's
resource-usage remarks only: no scratch, and the registers and LDS that give the occupancy DESIGN.md
4d states (three 192-thread blocks per CU at Cin = 256: 9 waves, up to 3 per SIMD).  The printed
figures are the ones in DESIGN.md's resource table."""
import os

import pytest

from stereoanywhere_amd._native import resource_usage

HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# template argument NKS = Cin / 32
KERNELS = {"mask_upsample_kernelILi2E": 64, "mask_upsample_kernelILi4E": 128, "mask_upsample_kernelILi8E": 256}
LDS_PER_CU = 160 * 1024


def test_mask_upsample_kernels_do_not_spill_and_keep_their_occupancy(tmp_path):
    usage = resource_usage("mask_upsample.hip", tmp_path)
    assert len(usage) == len(KERNELS), sorted(usage)
    for k, cin in KERNELS.items():
        (name, u), = [(n, v) for n, v in usage.items() if k in n]
        print(f"Cin {cin}: VGPRs {u['vgprs']} AGPRs {u['agprs']} scratch {u['scratch']} LDS {u['lds']} "
              f"occupancy {u['occupancy']}")
        assert u["scratch"] == 0, name
        # the split input of 48 pixels (Cin * 48 * 4 bytes) or the logits (144 x 60 floats), plus the bias
        # (and the padding between the two arrays)
        want = max(cin * 48 * 4, 144 * 60 * 4) + 144 * 4
        assert want <= u["lds"] <= want + 512, name
        # three blocks of three waves per CU: by LDS, and by registers (512 per SIMD lane, 3 waves)
        assert LDS_PER_CU // u["lds"] >= 3, name
        assert u["vgprs"] + u["agprs"] <= 168, name
        assert u["occupancy"] == 3, name

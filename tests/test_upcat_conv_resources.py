"""Compile-time check of the up-cat conv's backward kernels (hipcc for gfx950, no GPU), read from the
compile's resource-usage remarks only: no kernel of upcat_backward.hip uses scratch, and each kernel's LDS
bytes and occupancy are what DESIGN.md section 4k lists.  The printed VGPR figures are the ones there too."""
import os

import pytest

from stereoanywhere_amd._native import resource_usage

HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

TR = 4 * 32 * 64 * 4   # the dw transposition buffer: 32 sums x 64 lanes of fp32 per wave, 4 waves


def _pw(cx, cg, s, dx, dw):
    return f"pw_bwd_kernelILi{cx}ELi{cg}ELi{s}ELb{dx}ELb{dw}EE"


# kernel -> (LDS bytes per block, waves per SIMD); the dx-only instances keep no sums and no LDS
EXPECTED = {"up_adjoint_kernel": (2 * 4 * 256 * 4, 5), "pw_fold_kernel": (0, 8)}
for (cx, cg, s), occ in (((8, 8, 1), (4, 8, 4)), ((16, 16, 4), (3, 8, 4)), ((16, 8, 2), (4, 8, 4)),
                         ((32, 16, 4), (2, 7, 2))):
    for (dx, dw), o in zip(((1, 1), (1, 0), (0, 1)), occ):
        EXPECTED[_pw(cx, cg, s, dx, dw)] = (TR if dw else 0, o)


def test_upcat_backward_kernels_do_not_spill(tmp_path):
    usage = resource_usage("upcat_backward.hip", tmp_path)
    assert len(usage) == len(EXPECTED), sorted(usage)
    for k, (lds, occupancy) in EXPECTED.items():
        (name, u), = [(n, v) for n, v in usage.items() if k in n]
        print(f"{k}: VGPRs {u['vgprs']} AGPRs {u['agprs']} scratch {u['scratch']} LDS {u['lds']} "
              f"occupancy {u['occupancy']}")
        assert u["scratch"] == 0, name
        assert u["lds"] == lds, name
        assert u["occupancy"] == occupancy, name

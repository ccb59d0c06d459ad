"""Compile-time check of the split direct conv's instances (csrc/conv_direct.hip with the Makefile's
flags, no GPU): with the K-step pairs' 4 + 4 operand registers every instance still has no scratch
(spilled registers) and fits the waves per SIMD of its __launch_bounds__(512, DS ? 2 : 4).  Reads
only the compiler's resource summary."""
import os
import re

import pytest

from stereoanywhere_amd._native import resource_usage

HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# conv_direct_kernel<K, S, KC, NTL, DS, SP, CL>
INSTANCE = re.compile(r"conv_direct_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])E")
REGISTERS_PER_SIMD_LANE = 512   # gfx950: one file for VGPRs and AGPRs


def test_split_instances_do_not_spill_and_keep_their_occupancy(tmp_path):
    usage = resource_usage("conv_direct.hip", tmp_path)
    split = {}
    for name, u in usage.items():
        m = INSTANCE.search(name)
        if m and m.group(6) == "1":
            split[tuple(int(g) for g in m.groups())] = u
    print(split)
    # the stem, the 96-channel stride-2 conv plain and with the fused close, the 128-channel one
    assert len(split) == 4, sorted(usage)
    for (K, S, KC, NTL, DS, SP, CL), u in split.items():
        waves = 2 if DS else 4
        assert u["scratch"] == 0, (K, S, KC, NTL, DS, CL, u)
        assert u["vgprs"] + u["agprs"] <= REGISTERS_PER_SIMD_LANE // waves, (K, S, KC, NTL, DS, CL, u)
        assert u["occupancy"] >= waves, (K, S, KC, NTL, DS, CL, u)

"""Compile-time check of the any-geometry lookup + convc1 kernels (hipcc for gfx950, no GPU): their
64 accumulators stay in registers (no scratch), and the published (4, 4) instances are still
built beside them."""
import os

import pytest

from stereoanywhere_amd._native import resource_usage

HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.mark.parametrize("name,kernel,published", [
    ("corr_lookup.hip", "lookup_c1_fold_kernel", ["lookup_c1_vec_kernelILi4ELi4ELi64ELb0E", "lookup_c1_kernelILi4ELi4ELi64E"]),
    ("corr_shear.hip", "lookup_c1_shear_fold_kernel", ["lookup_c1_shear_lds_kernelILi4ELi4ELi64ELi8E"]),
])
def test_fold_kernels_do_not_spill(tmp_path, name, kernel, published):
    usage = resource_usage(name, tmp_path)
    new = {k: v for k, v in usage.items() if kernel in k}
    assert len(new) == 1, sorted(usage)
    (u,) = new.values()
    vgprs, scratch = u["vgprs"], u["scratch"]
    print(kernel, "VGPRs", vgprs, "scratch", scratch)
    assert scratch == 0
    # 64 accumulators + addressing: at least 4 waves per SIMD (512 VGPRs / 128)
    assert vgprs <= 128
    for p in published:
        assert any(p in k for k in usage), (p, sorted(usage))

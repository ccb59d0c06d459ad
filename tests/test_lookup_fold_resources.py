"""Compile-time check of the any-geometry lookup + convc1 kernels (hipcc for gfx950, no GPU): their
64 accumulators stay in registers (no scratch), and the published (4, 4) instances are still
built beside them."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereoanywhere_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _usage(name, tmp_path):
    """{kernel: (VGPRs, scratch bytes per lane)} from the compile's resource-usage remarks."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, name), "-o", str(tmp_path / "k.o")]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur, vgprs = {}, None, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r" VGPRs: (\d+)", line)
        if m:
            vgprs = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            out[cur] = (vgprs, int(m.group(1)))
    return out


@pytest.mark.parametrize("name,kernel,published", [
    ("corr_lookup.hip", "lookup_c1_fold_kernel", ["lookup_c1_vec_kernelILi4ELi4ELi64ELb0E", "lookup_c1_kernelILi4ELi4ELi64E"]),
    ("corr_shear.hip", "lookup_c1_shear_fold_kernel", ["lookup_c1_shear_lds_kernelILi4ELi4ELi64ELi8E"]),
])
def test_fold_kernels_do_not_spill(tmp_path, name, kernel, published):
    usage = _usage(name, tmp_path)
    new = {k: v for k, v in usage.items() if kernel in k}
    assert len(new) == 1, sorted(usage)
    (vgprs, scratch), = new.values()
    print(kernel, "VGPRs", vgprs, "scratch", scratch)
    assert scratch == 0
    # 64 accumulators + addressing: at least 4 waves per SIMD (512 VGPRs / 128)
    assert vgprs <= 128
    for p in published:
        assert any(p in k for k in usage), (p, sorted(usage))

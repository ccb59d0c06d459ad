"""Compile-time check of the fused training-loss kernels (hipcc for gfx950, no GPU), read from the
compile's resource-usage remarks only: no kernel of losses.hip uses scratch (the maps of a launch
are indexed in the kernel arguments, not in a private copy) and each stays within 64 KiB of LDS.  The
printed VGPR / LDS / occupancy figures are the ones in DESIGN.md section 4g."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereoanywhere_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

KERNELS = ["loss_stats_kernel", "loss_fwd_kernel", "loss_finalise_kernel", "loss_bwd_kernel"]


def _usage(name, tmp_path):
    """{kernel: {field: value}} from the compile's resource-usage remarks."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, name), "-o", str(tmp_path / "k.o")]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    fields = {"vgprs": r" VGPRs: (\d+)", "agprs": r" AGPRs: (\d+)",
              "scratch": r"ScratchSize \[bytes/lane\]: (\d+)", "occupancy": r"Occupancy \[waves/SIMD\]: (\d+)",
              "lds": r"LDS Size \[bytes/block\]: (\d+)"}
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
        for key, pat in fields.items():
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def test_loss_kernels_do_not_spill(tmp_path):
    usage = _usage("losses.hip", tmp_path)
    assert len(usage) == len(KERNELS), sorted(usage)
    for k in KERNELS:
        (name, u), = [(n, v) for n, v in usage.items() if k in n]
        print(f"{k}: VGPRs {u['vgprs']} AGPRs {u['agprs']} scratch {u['scratch']} LDS {u['lds']} "
              f"occupancy {u['occupancy']}")
        assert u["scratch"] == 0, name
        assert u["lds"] <= 64 * 1024, name

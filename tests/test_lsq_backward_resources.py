"""Compile-time check of the softlrc / weighted_lsq backward kernels (hipcc for gfx950, no GPU), read
from the compile's resource-usage remarks only: every kernel of lsq_backward.hip runs without scratch.
The printed VGPR / LDS / occupancy figures are the ones in DESIGN.md section 4f.  The forward of the
differentiable weighted_lsq (lsq_stats.hip) is the second instance of the inference kernel: it must
use what the first one (lsq.hip) uses, no more."""
import os

import pytest

from stereoanywhere_amd._native import resource_usage

HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

KERNELS = ["lrcb_px_kernel", "lrcb_gather_kernel", "lsqb_kernel"]


def _show(k, u):
    print(f"{k}: VGPRs {u['vgprs']} AGPRs {u['agprs']} scratch {u['scratch']} LDS {u['lds']} occupancy {u['occupancy']}")


def test_backward_kernels_do_not_spill(tmp_path):
    usage = resource_usage("lsq_backward.hip", tmp_path)
    assert len(usage) == len(KERNELS), sorted(usage)
    for k in KERNELS:
        (name, u), = [(n, v) for n, v in usage.items() if k in n]
        _show(k, u)
        assert u["scratch"] == 0, name
        assert u["lds"] <= 64 * 1024, name


def test_stats_instance_uses_what_the_inference_instance_uses(tmp_path):
    (stats, s), = resource_usage("lsq_stats.hip", tmp_path).items()
    (infer, i), = [(n, v) for n, v in resource_usage("lsq.hip", tmp_path).items() if "lsq1_kernel" in n]
    assert "lsq1_kernelILb1E" in stats and "lsq1_kernelILb0E" in infer
    _show("lsq1_kernel<true>", s)
    _show("lsq1_kernel<false>", i)
    for key in ("vgprs", "agprs", "scratch", "lds", "occupancy"):
        assert s[key] == i[key], key

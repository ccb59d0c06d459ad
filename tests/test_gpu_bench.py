"""bench.py's plain run end to end on the GPU, at the graph tests' size (2 pairs of 128x256): the
line carries the headline keys and none of the --full ones, --steps sets the timed steps, and
--dump-outputs writes what the forward returns on the seeded inputs.  One bench process serves
both tests."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, ITERS, STEPS = 2, 128, 256, 4, 3


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--batch", str(B), "--height", str(H), "--width", str(W),
                        "--iters", str(ITERS), "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), d, r.stderr


def test_plain_run_reports_the_headline_only(plain):
    line, _, err = plain
    assert line["unit"] == "pairs/s" and line["higher_is_better"] is True and line["n_gpus"] == 1
    assert isinstance(line["metric"], str) and line["dtype"].startswith("f32")
    assert line["steps"] == STEPS and f"timed {STEPS} steps" in err
    # value and ms_per_step describe the same timed region: B pairs per step
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(B / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["full"] is False
    for k in ("roofline", "cpu_baseline", "epe_vs_reference", "box_state", "eager_ms_per_step",
              "graph_vs_eager_max_abs"):
        assert k not in line, k
    for leg in ("one-stream steps", "instrumented", "cpu baseline", "EPE vs reference"):
        assert leg not in err, leg


def test_dump_is_the_forward_on_the_seeded_inputs(plain):
    """The replayed graph (or the eager launches the probe chose) computes the eager forward bit for
    bit (bench.py --full refuses a line otherwise), so the dump equals this process's forward."""
    import bench
    from stereoanywhere_amd import synth
    from stereoanywhere_amd.model import StereoAnywhere

    _, d, _ = plain
    assert sorted(os.listdir(d)) == ["flow_up.npy"]
    got = np.load(os.path.join(d, "flow_up.npy"))
    assert got.dtype == np.float32 and got.shape == (B, 1, H, W) and np.isfinite(got).all()
    torch.backends.cudnn.benchmark = False
    m = StereoAnywhere(dict(bench.PUBLISHED)).eval()
    synth.load_seeded_weights(m, 0)
    m = m.cuda()
    inp = bench.make_inputs(B, H, W, H, W, 192.0, seed0=1, device="cuda")
    with torch.no_grad():
        ref = m(inp["left"], inp["right"], inp["mono_left"], inp["mono_right"], iters=ITERS, test_mode=True)[0]
    np.testing.assert_array_equal(got, ref.cpu().numpy())

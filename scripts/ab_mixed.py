#!/usr/bin/env python3
"""Default vs mixed precision (model.mixed_precision: the F(4x4) convs' single-f16-operand kernel,
block_shape 7) at bench.py's plain config: B=4 pairs 544x960, 22 iterations, ForwardGraph replay.
Alternates default / mixed (three rounds by default), then once per mode: the conv2d_wino4 total
from the timing API (one-stream eager steps, as bench.py measures its per-kernel times), the range
guards' redo count and the EPE against tests/golden/cfg2_544x960_it22.npz.
usage: python scripts/ab_mixed.py [steps] [rounds]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from stereoanywhere_amd import _native as N  # noqa: E402
from stereoanywhere_amd import ops, synth  # noqa: E402
from stereoanywhere_amd.graph import ForwardGraph  # noqa: E402
from stereoanywhere_amd.model import StereoAnywhere  # noqa: E402

MODES = (("default", False), ("mixed", True))


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    dev = torch.device("cuda", 0)
    model = StereoAnywhere(dict(bench.PUBLISHED)).eval()
    synth.load_seeded_weights(model, 0)
    model = model.to(dev)
    inp = bench.make_inputs(4, 540, 960, 544, 960, 192.0, seed0=1, device=dev)
    x = [inp["left"], inp["right"], inp["mono_left"], inp["mono_right"]]
    graphs = {name: ForwardGraph(model) for name, _ in MODES}   # one capture per mode, kept
    with torch.no_grad():
        for name, mixed in MODES:   # capture + warm-up
            model.mixed_precision = mixed
            graphs[name](*x, iters=22)
            graphs[name](*x, iters=22)
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in MODES}
        for rnd in range(rounds):
            for name, mixed in MODES:
                model.mixed_precision = mixed
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    graphs[name](*x, iters=22)
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / steps * 1e3)
                print(f"round {rnd} {name}: {ms[name][-1]:.2f} ms/step ({steps} graph replays)", flush=True)
        for name, mixed in MODES:
            model.mixed_precision = mixed
            model.stream_overlap = False
            model(*x, iters=22, test_mode=True)
            N.lib().sa_split_redo_blocks(1)
            ops.W4_SHAPE_LAUNCHES.clear()
            N.timing_enable(True)
            torch.cuda.synchronize()
            for _ in range(3):
                model(*x, iters=22, test_mode=True)
            torch.cuda.synchronize()
            w4_ms, w4_n = N.timing_read("conv2d_wino4")
            N.timing_enable(False)
            model.stream_overlap = True
            redo = int(N.lib().sa_split_redo_blocks(1))
            shapes = dict(ops.W4_SHAPE_LAUNCHES)
            epe = bench.epe_vs_reference(model, dev)
            print(f"{name}: {min(ms[name]):.2f} / {sorted(ms[name])[len(ms[name]) // 2]:.2f} ms/step (min / median of "
                  f"{rounds}); conv2d_wino4 {w4_ms / 3:.2f} ms/step in {w4_n // 3} launches (one-stream eager, "
                  f"timing API); F(4x4) launches by block shape (3 steps) {shapes}; sa_split_redo_blocks {redo}; "
                  f"EPE vs cfg2_544x960_it22 {epe:.3e}", flush=True)
        model.mixed_precision = False
        a, b = min(ms["default"]), min(ms["mixed"])
        print(f"mixed / default (min ms/step): {b / a:.4f}")


if __name__ == "__main__":
    main()

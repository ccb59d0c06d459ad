"""Replica, rerun, dirty-memory and two-stream bit-equality of conv3d_k3's kernels (tests/invariance_util.py):
the forward and the data gradient on sa_conv3d_mf_scaled with sa_sample_scale's per-sample scales, and
sa_conv3d_k3_backward_weight with its float64 work buffer, which is an output here.  One seeded sample (sample 0
of a case of tests/conv3d_k3_ref.py) is replicated along the batch; identical samples in different blocks must
give identical bits (P1), three calls the same bits (P2) whatever the destinations, the work buffer and the
allocator's free blocks held before (P3), two streams at once the serial bits (P4).  Replica 0 is checked
against the float64 reference at its own test's tolerance.  dw sums over the batch and has no batch position:
P1 does not apply to it, its oracle is R x the sample's float64 dw."""
import pytest
import torch

import conv3d_k3_ref as R
from invariance_util import Case, run_case
from stereoanywhere_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = {8: R.SHAPES[0], 16: R.SHAPES[2], 32: R.SHAPES[5]}


def conv_case(C, what):
    """what "out": conv(x, w) with x scaled per sample; "dx": conv(g, flipped w) likewise."""
    c = R.case(*SHAPES[C])
    v, w, ref = ((c["x"], c["weight"], c["out"]) if what == "out" else (c["g"], R.flipped(c["weight"]), c["dx"]))

    def inputs(rep):
        return {"v": rep(v[:1]), "w_t": R.to_taps(w).cuda()}

    def call(inp, d):
        return (ops.conv3d_mf_scaled(inp["v"], ops.conv3d_mf_table(inp["w_t"]), *ops.sample_scale(inp["v"], C)),)

    def oracle(inp, outs):
        e = float((outs[0][:1].double().cpu() - ref[:1]).abs().max() / ref[:1].abs().max())
        assert e < 2e-6, e

    return Case(f"conv3d_k3[{C}, {what}]", inputs, call, oracle, streams=True)


def dw_case(C):
    c = R.case(*SHAPES[C])
    x, g = c["x"][:1], c["g"][:1]
    _, dw1 = R.grads(x.double(), c["weight"].double(), g.double())
    _, mag1 = R.grads(x.double().abs(), c["weight"].double(), g.double().abs())

    def inputs(rep):
        return {"x": rep(x), "g": rep(g)}

    def dests(inp):
        return (torch.empty(ops.conv3d_k3_backward_weight_work(C, *[inp["x"].shape[i] for i in (0, 2, 3, 4)]),
                            device="cuda", dtype=torch.float64),)

    def call(inp, d):
        dw = ops.conv3d_k3_backward_weight(inp["x"], inp["g"], None, ops.sample_scale(inp["g"], 1)[0], work=d[0])
        return (dw[None], d[0][None])

    def oracle(inp, outs):
        reps = inp["x"].shape[0]
        got = R.from_taps(outs[0][0]).double().cpu()
        assert bool(((got - reps * dw1).abs() <= R.dw_bound(reps * mag1)).all())
        assert bool(outs[1].isfinite().all())   # every entry of the poisoned work buffer was written

    return Case(f"conv3d_k3_backward_weight[{C}]", inputs, call, oracle, dests=dests, streams=True, p1=False)


CASES = [conv_case(C, what) for C in SHAPES for what in ("out", "dx")] + [dw_case(C) for C in SHAPES]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_invariance(case):
    run_case(case)

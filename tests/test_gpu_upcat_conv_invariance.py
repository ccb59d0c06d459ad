"""Replica, rerun and dirty-memory bit-equality of the up-cat conv's kernels (tests/invariance_util.py):
sa_trilinear_up_adjoint, sa_conv3d_pointwise_backward (dx and dw, its float64 work buffer poisoned with the
destinations) and the forward instance <16, 16, identity a> of sa_conv3d_pointwise_upcat that training
uses.  One seeded sample (sample 0 of a case of tests/upcat_conv_ref.py) is replicated along the batch;
identical samples in different blocks must give identical bits (P1), three calls the same bits (P2) whatever
the destinations, the work buffer and the allocator's free blocks held before (P3).  Each case also checks
replica 0 against the float64 reference at its own test's tolerance.  dw sums over the batch and has no
batch position: P1 does not apply to it, its oracle is R x the sample's float64 dw."""
import pytest
import torch

import hourglass_ref as HR
import upcat_conv_ref as R
from invariance_util import Case, run_case
from test_gpu_hourglass_ref import _upcat_bound
from stereoanywhere_amd import ops

pytestmark = pytest.mark.gpu

FULL, LOW = R.SHAPES[2]   # (10, 7, 67) <- (3, 2, 20): a factor above 2, inexact scales, W % 4 != 0


def _close(key, got, c):
    m, allowed = R.metric(got[:1], c["ref"][key][:1]), R.allowance(c, key)
    assert m <= allowed, (key, m, allowed)


def adjoint_case(triple, low_first):
    c = R.case(FULL, LOW, triple, low_first)

    def dests(inp):
        return (torch.empty((inp["g"].shape[0], triple[2]) + LOW, device="cuda"),)

    return Case(f"trilinear_up_adjoint[{triple[2]} channels]", lambda rep: {"g": rep(c["g"][:1])},
                lambda inp, d: (ops.trilinear_up_adjoint(inp["g"], LOW, out=d[0]),),
                lambda inp, outs: _close("dp", outs[0], c), dests=dests)


def backward_case(triple, low_first, branch, what):
    """branch "a": (skip, g, w_a), the pair (Ca, Cout); branch "u": (low, dp, w_u), the pair (Cu, Cout)."""
    c = R.case(FULL, LOW, triple, low_first)
    w_a, w_u = R.split(c["weight"], triple[0], low_first)
    x, g, w, key = ((c["skip"], c["g"], w_a, "da") if branch == "a" else
                    (c["low"], c["ref"]["dp"].float(), w_u, "du"))
    x, g = x[:1], g[:1]

    def inputs(rep):
        return {"x": rep(x), "g": rep(g), "w": w.cuda()}

    def dests(inp):
        B, cx = inp["x"].shape[:2]
        n = inp["x"][0, 0].numel()
        work = torch.empty(ops.conv3d_pointwise_backward_work(cx, inp["g"].shape[1], B, n), device="cuda",
                           dtype=torch.float64)
        return (torch.empty_like(inp["x"]), work)

    def call(inp, d):
        dx, dw = ops.conv3d_pointwise_backward(inp["x"], inp["g"], inp["w"], what != "dw", what != "dx", out=d[0],
                                               work=d[1])
        return (dx,) if what == "dx" else (dw[None],)

    def oracle(inp, outs):
        if what == "dx":
            return _close(key, outs[0], c)
        # a lane adds at most 32 fp32 products, everything above is float64: (32 + 2) u on the magnitude
        reps = inp["x"].shape[0]
        ref = reps * torch.einsum("bcdhw,bodhw->co", x.double(), g.double())
        mag = reps * torch.einsum("bcdhw,bodhw->co", x.double().abs(), g.double().abs())
        assert bool(((outs[0][0].double().cpu() - ref).abs() <= 34 * HR.U * mag).all())

    cx, cg = x.shape[1], g.shape[1]
    return Case(f"conv3d_pointwise_backward[{cx} x {cg}, {what}]", inputs, call, oracle, dests=dests, p1=what == "dx")


def forward_case():
    """sa_conv3d_pointwise_upcat <16, 16, identity a>: two launches (p is a torch.empty workspace)."""
    triple, low_first = R.TRIPLES[1]
    c = R.case(FULL, LOW, triple, low_first)
    w_a, w_u = R.split(c["weight"], triple[0], low_first)

    def inputs(rep):
        return {"a": rep(c["skip"][:1]), "u": rep(c["low"][:1]), "wa": w_a.cuda(), "wu": w_u.cuda()}

    def call(inp, d):
        return (ops.conv3d_pointwise_upcat(ops.VolAct(inp["a"]), ops.VolAct(inp["u"]), inp["wa"], inp["wu"], 16,
                                           stats=False).raw,)

    def oracle(inp, outs):
        ref, m = HR.upcat(c["skip"][:1].double(), c["low"][:1].double(), w_a, w_u)
        assert bool(((outs[0][:1].double().cpu() - ref).abs() <= _upcat_bound(16, 32, m)).all())

    return Case("conv3d_pointwise_upcat[16x16 identity a]", inputs, call, oracle)


CASES = [adjoint_case(*R.TRIPLES[0]), adjoint_case(*R.TRIPLES[1]), forward_case()] + [
    backward_case(t, lf, branch, what) for t, lf in R.TRIPLES for branch in "au" for what in ("dx", "dw")]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_invariance(case):
    run_case(case)

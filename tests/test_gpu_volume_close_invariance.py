"""Replica, rerun and dirty-memory bit-equality of the hourglass close (tests/invariance_util.py): the
statistics pass, the backward's reduce launch (gate gradients only, so the apply launch is skipped) and
the whole backward with its apply launch, gated and gate-less.  One seeded sample of shape
(1, 2, 5, 3, 70) is replicated along the batch; identical samples in different blocks must give identical
bits (P1), three calls the same bits (P2) whatever the destinations, the partial buffers and the
allocator's free blocks held before (P3).  Each case also checks replica 0 against the float64 reference
at its own test's tolerance."""
import pytest
import torch

import volume_close_ref as R
from invariance_util import Case, run_case
from stereoanywhere_amd import ops

pytestmark = pytest.mark.gpu

SHAPE = (1, 2, 5, 3, 70)


def _close(key, got, c):
    m, allowed = R.metric(got[:1], c["ref"][key]), R.allowance(c, key)
    assert m <= allowed, (key, m, allowed)


def _gate(key, got, c, terms):
    bound = (terms + 4) * R.U * c["mag_l" if key == "dgl" else "mag_r"]
    assert bool(((got[:1].double().cpu() - c["ref"][key]).abs() <= bound).all()), key


def _inputs(c, gated):
    def inputs(rep):
        inp = {k: rep(c[k]) for k in ("x", "g") + (("gl", "gr") if gated else ())}
        B = inp["x"].shape[0]
        # the sample's statistics (the reference's, rounded to fp32), one [B*C] vector for all replicas
        inp["mean"], inp["rstd"] = (c["ref"][k].float().cuda().repeat(B) for k in ("mean", "rstd"))
        return inp
    return inputs


def stats_case():
    c = R.case(SHAPE, False)

    def call(inp, dests):
        B, C = inp["x"].shape[:2]
        mean, rstd = ops.volume_close_stats(inp["x"], R.EPS)
        return mean.reshape(B, C), rstd.reshape(B, C)

    def oracle(inp, outs):
        for key, got in zip(("mean", "rstd"), outs):
            m, allowed = R.metric(got[0], c["ref"][key]), R.allowance(c, key)
            assert m <= allowed, (key, m, allowed)

    return Case("volume_close_stats", lambda rep: {"x": rep(c["x"])}, call, oracle)


def backward_case(gated, need_x):
    c = R.case(SHAPE, gated)

    def dests(inp):
        return (torch.empty_like(inp["x"]),) if need_x else ()

    def call(inp, dests):
        dx, dgl, dgr = ops.volume_close_backward(inp["g"], inp["x"], inp["mean"], inp["rstd"], inp.get("gl"),
                                                 inp.get("gr"), R.SLOPE, need_x, gated, gated,
                                                 out=dests[0] if need_x else None)
        return tuple(t for t in (dx, dgl, dgr) if t is not None)

    def oracle(inp, outs):
        outs = list(outs)
        if need_x:
            _close("dx", outs.pop(0), c)
        if gated:
            _gate("dgl", outs[0], c, SHAPE[2])
            _gate("dgr", outs[1], c, SHAPE[4])

    what = "reduce + apply" if need_x else "reduce"
    return Case(f"volume_close_backward {what}{', gated' if gated else ''}", _inputs(c, gated), call, oracle,
                dests=dests)


CASES = [stats_case(), backward_case(True, False), backward_case(True, True), backward_case(False, True)]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_invariance(case):
    run_case(case)

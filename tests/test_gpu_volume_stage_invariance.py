"""Replica, rerun and dirty-memory bit-equality of the volume stage (tests/invariance_util.py): each
kind with and without the truncation, and the truncation's backward.  One seeded sample is replicated
along the batch; identical samples in different blocks must give identical bits (P1), three calls the
same bits (P2) whatever the destination, the maximum's workspace and the allocator's free blocks held
before (P3).  Each case also checks replica 0 against the restatement at its own test's tolerance."""
import pytest
import torch

import volume_stage_ref as R
from invariance_util import Case, run_case
from stereoanywhere_amd import ops

pytestmark = pytest.mark.gpu

H, W = 3, 37          # odd rows, a scalar tail
NBINS, BIN, SHIFT, ATTEN = 4, 1, 36, 0.9
KEYS = ("volume", "mde", "noise", "disp", "conf")


def stage_case(kind, trunc):
    c = R.random_case(21, 1, H, W, W)

    def inputs(rep):
        return {k: rep(c[k].float()) for k in KEYS}

    def dests(inp):
        return (torch.empty_like(inp["volume"]),)

    def call(inp, dests):
        kw = dict(kind=kind, nbins=NBINS, bin=BIN, shift=SHIFT, out=dests[0])
        if kind != "none":
            kw["mde"] = inp["mde"]
        if kind == "noise":
            kw["noise"] = inp["noise"]
        if kind == "zero":
            kw["peak"] = ops.volume_peak(inp["volume"])
        if trunc:
            kw.update(trunc_disp=inp["disp"], trunc_conf=inp["conf"], atten=ATTEN)
        return (ops.volume_stage(inp["volume"], **kw),)

    def oracle(inp, outs):
        t = (c["disp"], c["conf"], ATTEN) if trunc else None
        got = outs[0][:1].cpu()
        if kind == "zero" or trunc:
            R.assert_close(got, R.stage(c["volume"], kind, c["mde"], NBINS, BIN, SHIFT, c["noise"], t, torch.float64),
                           f"{kind} trunc {trunc}")
        else:
            assert torch.equal(got, R.stage(c["volume"], kind, c["mde"], NBINS, BIN, SHIFT, c["noise"]))

    return Case(f"volume_stage {kind}{' + truncation' if trunc else ''}", inputs, call, oracle, dests=dests)


def backward_case():
    c = R.random_case(22, 1, H, W, W)

    def inputs(rep):
        return {k: rep(c[k].float()) for k in ("volume", "disp", "conf")}

    def dests(inp):
        return (torch.empty_like(inp["volume"]),)

    def call(inp, dests):
        return (ops.volume_truncate_backward(inp["volume"], inp["disp"], inp["conf"], ATTEN, out=dests[0]),)

    def oracle(inp, outs):
        f64 = R.trunc_factor(c["disp"], c["conf"], ATTEN, W, torch.float64)
        R.assert_close(outs[0][:1].cpu(), c["volume"].double() * f64, "truncate backward")

    return Case("volume_truncate_backward", inputs, call, oracle, dests=dests)


CASES = [stage_case(kind, trunc) for kind in ("none", "roll", "noise", "zero") for trunc in (False, True)
         if kind != "none" or trunc] + [backward_case()]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_invariance(case):
    run_case(case)

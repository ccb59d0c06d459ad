"""The split direct conv with K-steps paired on v_mfma_f32_16x16x32_f16 (csrc/conv_direct.hip) against
a float64 torch conv computed on the CPU, at the smallest shapes that reach what the pairing can
break: N = 2, 9 x 33 outputs (two 8 x 32 tiles in each direction, the second one pixel wide / high,
zero padding on all four borders), every (K, S, Cout) the dispatch table builds, two chunks of input
channels, a single zero-padded chunk (Cin not a multiple of the chunk), and the 7x7 stem's odd
number of K-steps (49: 24 pairs and one 16x16x16 step).

Tolerance: the one tests/test_gpu_direct.py applies to the split form (read from that file below).
It holds for these shapes with room to spare: the products are exact, the sums run in fp32 over at
most 16 * 9 + 16 terms of magnitude <= 1, so the error is a few 1e-7 against atol 2e-5.

Range guard: image 1 is (|randn| + 1) * 2^16, every value past the documented envelope of the split
(|x| < 65504: 65520 rounds to an f16 infinity), so every block of that image is recomputed on fp32
MFMA products; its weights are |randn| scaled, so no sum cancels and the relative part of the
tolerance covers both kernels' fp32 rounding (<= 160 * 2^-24 = 1e-5 of the result) at outputs of
1e5 and more.  The data are finite and so is the float64 reference (checked): this is the kernel's
intended recovery path."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from invariance_util import Case, run_case
from stereoanywhere_amd import _native as N, ops

pytestmark = pytest.mark.gpu
dev = "cuda"

_SRC = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_direct.py")).read()
_TOL = re.search(r"assert_close\(out, ref, atol=([0-9.e-]+), rtol=([0-9.e-]+)\)", _SRC)
assert _TOL, "tests/test_gpu_direct.py no longer states the split form's tolerance"
TOL = dict(atol=float(_TOL.group(1)), rtol=float(_TOL.group(2)))

# (K, S, Cout, Cin): conv_direct.hip's pick(); Cin 8 / 16 = two chunks (KC = 4 / 8), 3 / 5 = one padded chunk
CONFIGS = [(7, 1, 64, 8), (7, 1, 64, 3), (7, 1, 128, 3),
           (3, 2, 96, 16), (3, 2, 96, 5), (3, 2, 128, 16), (3, 2, 128, 5), (3, 2, 256, 16), (3, 2, 256, 5)]
HO, WO = 9, 33


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def problem(K, S, Cout, Cin, seed=0):
    """(x, w, wd) on the CPU: N = 2, the input size whose output is 9 x 33."""
    H, W = (HO, WO) if S == 1 else (2 * HO, 2 * WO - 1)
    x = rnd(2, Cin, H, W, seed=seed + 1)
    w = rnd(Cout, Cin, K, K, seed=seed + 2) / (K * Cin ** 0.5)
    wd = rnd(Cout, Cin, 1, 1, seed=seed + 3) / Cin ** 0.5 if S == 2 else None
    return x, w, wd


def reference(x, w, wd, K, S):
    """float64 on the CPU: (conv, downsample or None)."""
    ref = F.conv2d(x.double(), w.double(), stride=S, padding=K // 2)
    assert ref.shape[2:] == (HO, WO)
    return ref, (F.conv2d(x.double(), wd.double(), stride=S) if wd is not None else None)


def arranged(w, wd, S, split):
    saved, ops.DIRECT_SPLIT = ops.DIRECT_SPLIT, split
    try:
        wg_ = ops.conv_direct_weights(w.to(dev), S)
        wd_ = None if wd is None else ops.conv_direct_weights(wd.to(dev), S, with_ds=True)
    finally:
        ops.DIRECT_SPLIT = saved
    assert (wg_.dtype == torch.int32) == split
    return wg_, wd_


def check(got, ref64, what):
    got = got.cpu()
    err = (got.double() - ref64).abs()
    print(f"{what}: max abs error {float(err.max()):.3g}, max |ref| {float(ref64.abs().max()):.3g}")
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, ref64.float(), **TOL)


@pytest.mark.parametrize("K,S,Cout,Cin", CONFIGS)
def test_paired_split_matches_float64(K, S, Cout, Cin):
    """Both outputs of every built configuration, and the InstanceNorm means from the statistics
    partials (tests/test_gpu_direct.py's bound for them)."""
    x, w, wd = problem(K, S, Cout, Cin)
    ref, ref_d = reference(x, w, wd, K, S)
    wg_, wd_ = arranged(w, wd, S, True)
    N.lib().sa_split_redo_blocks(1)
    res = ops.conv_direct(x.to(dev), wg_, K, S, Cout, wd=wd_, stats=True)
    check(res[0], ref, f"K{K} S{S} {Cin}->{Cout} conv")
    torch.testing.assert_close(res[-1][0][0].cpu(), ref.mean(dim=(2, 3)).flatten().float(), atol=1e-5, rtol=1e-5)
    if S == 2:
        check(res[1], ref_d, f"K{K} S{S} {Cin}->{Cout} downsample")
        torch.testing.assert_close(res[-1][1][0].cpu(), ref_d.mean(dim=(2, 3)).flatten().float(), atol=1e-5, rtol=1e-5)
    assert int(N.lib().sa_split_redo_blocks(1)) == 0


def _partials(monkeypatch):
    """ops.instnorm_finalize also records the partial sums the conv's blocks wrote."""
    got, real = [], ops.instnorm_finalize

    def spy(partial, *a, **k):
        got.append(partial)
        return real(partial, *a, **k)
    monkeypatch.setattr(ops, "instnorm_finalize", spy)
    return got


def test_fused_close_equals_norm_act_then_conv(monkeypatch):
    """The close instance against ops.norm_act followed by the plain split conv of the same build:
    outputs, statistics partials and finalized statistics bit for bit; and against float64."""
    Cin, Cout = 16, 96
    _, w, wd = problem(3, 2, Cout, Cin)
    c2 = (rnd(2, Cin, 2 * HO, 2 * WO - 1, seed=6) * 3 + 0.5).to(dev)
    skip = torch.relu(rnd(2, Cin, 2 * HO, 2 * WO - 1, seed=7)).to(dev)
    mean, rstd = (rnd(2 * Cin, seed=8) * 0.3).to(dev), (rnd(2 * Cin, seed=9).abs() + 0.2).to(dev)
    wg_, wd_ = arranged(w, wd, 2, True)
    y = ops.norm_act(c2, ops.Affine(mean, rstd, None, per_plane=True), act_in="relu", skip=skip, act_out="relu")
    parts = _partials(monkeypatch)
    ref = ops.conv_direct(y, wg_, 3, 2, Cout, wd=wd_, stats=True)
    got = ops.conv_direct(c2, wg_, 3, 2, Cout, wd=wd_, stats=True, close=(skip, mean, rstd))
    assert len(parts) == 4
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert torch.equal(parts[0], parts[2]) and torch.equal(parts[1], parts[3])
    for (m0, r0), (m1, r1) in zip(got[2], ref[2]):
        assert torch.equal(m0, m1) and torch.equal(r0, r1)
    r64, r64d = reference(y.cpu(), w, wd, 3, 2)
    check(got[0], r64, "close conv")
    check(got[1], r64d, "close downsample")


@pytest.mark.parametrize("K,S,Cout,Cin", [(7, 1, 64, 3), (3, 2, 96, 16), (3, 2, 128, 16)])
def test_range_guard_redo(K, S, Cout, Cin):
    x, w, wd = problem(K, S, Cout, Cin)
    x[1] = (x[1].abs() + 1) * 65536.0   # every value >= 65536 > 65520: past the split's envelope
    w, wd = w.abs(), (wd.abs() if wd is not None else None)
    ref, ref_d = reference(x, w, wd, K, S)
    assert torch.isfinite(ref).all() and torch.isfinite(ref.float()).all()
    outs = {}
    for split in (False, True):
        wg_, wd_ = arranged(w, wd, S, split)
        N.lib().sa_split_redo_blocks(1)
        res = ops.conv_direct(x.to(dev), wg_, K, S, Cout, wd=wd_)
        outs[split] = ([r.cpu() for r in res], int(N.lib().sa_split_redo_blocks(1)))
    (ys, redo), (yf, redo_f) = outs[True], outs[False]
    print(f"K{K} S{S} {Cin}->{Cout}: {redo} blocks redone")
    assert redo >= 1 and redo_f == 0
    check(ys[0], ref, "guarded conv vs float64")
    torch.testing.assert_close(ys[0], yf[0], **TOL)
    if S == 2:
        check(ys[1], ref_d, "guarded downsample vs float64")
        torch.testing.assert_close(ys[1], yf[1], **TOL)


@pytest.mark.parametrize("form,K,S,Cout,Cin", [("stem", 7, 1, 64, 3), ("s2", 3, 2, 96, 16), ("close", 3, 2, 96, 16),
                                               ("s2", 3, 2, 128, 16)])
def test_rerun_and_dirty_memory_equality(form, K, S, Cout, Cin):
    """invariance_util.run_case: the call on memory poisoned with NaN words, zeros and NaN words
    again gives the same bits each time, the same for both replicas, and a result that matches
    float64."""
    x, w, wd = problem(K, S, Cout, Cin)
    x = x[:1] * 3 + 0.5 if form == "close" else x[:1]
    skip = torch.relu(rnd(1, Cin, *x.shape[2:], seed=7))
    mean, rstd = rnd(1, Cin, seed=8) * 0.3, rnd(1, Cin, seed=9).abs() + 0.2

    def inputs(rep):
        wg_, wd_ = arranged(w, wd, S, True)
        return rep(x), wg_, wd_, rep(skip), rep(mean).reshape(-1), rep(rstd).reshape(-1)

    def call(inp, dests):
        xs, wg_, wd_, sk, m, r = inp
        res = ops.conv_direct(xs, wg_, K, S, Cout, wd=wd_, stats=True, close=(sk, m, r) if form == "close" else None)
        B = xs.shape[0]
        return tuple(res[:-1]) + tuple(t.view(B, -1) for st in res[-1] for t in st)

    def oracle(inp, outs):
        xin = x
        if form == "close":
            xin = torch.relu(torch.relu((x - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)) + skip)
        ref, ref_d = reference(xin, w, wd, K, S)
        check(outs[0][:1], ref, f"{form} {Cout} conv")
        if S == 2:
            check(outs[1][:1], ref_d, f"{form} {Cout} downsample")

    run_case(Case(f"direct_k32[{form} {Cout}]", inputs, call, oracle, R=2))

"""The HIP adjoints of softlrc and weighted_lsq (csrc/lsq_backward.hip, lsq_stats.hip) through
ops.softlrc_backward / ops.weighted_lsq_stats / ops.weighted_lsq_backward, against torch.autograd of the
reference formulation in float64 (tests/lsq_lrc_ref.py) from the same fp32 inputs.

The yardstick is the one of tests/test_gpu_diffops_backward.py, the reference formulation's own fp32
autograd on the CPU: with e_ref = max |grad_fp32_torch - grad_fp64|, each gradient tensor must satisfy
max |grad_hip - grad_fp64| <= 4 e_ref.  Every case is run twice: the two results must be the same bits.

softlrc's inputs are built away from the kinks of bilinear sampling, |u| and relu (lsq_lrc_ref.lrc_inputs;
the precondition is asserted for every pixel and no pixel is left out of the comparison).  The float64
restatement of weighted_lsq takes its band from torch.quantile of the fp32 values, as the reference's
.float() does; only the solve is float64."""
import functools

import numpy as np
import pytest
import torch

import lsq_lrc_ref as ref
from stereoanywhere_amd import ops

pytestmark = pytest.mark.gpu
dev = "cuda"


def g(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def c(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _check(label, got, want64, want32):
    e_ref = np.abs(want32 - want64).max()
    err = np.abs(got.astype(np.float64) - want64).max()
    mag = np.abs(want64).max()
    print(f"{label}: err {err:.3g}, e_ref {e_ref:.3g} ({e_ref / mag:.2g} of max|g|), err/e_ref {err / e_ref:.3g}")
    assert np.isfinite(got).all(), label
    assert err <= 4 * e_ref, label


# ------------------------------------------------------------------------------------ softlrc
# a single row; odd sizes; a width past one wave
SHAPES = [(1, 2), (5, 7), (9, 33), (3, 65)]
USE = {"s2": (1, 0), "s3": (0, 1), "both": (1, 1)}
B = 2


@functools.lru_cache(maxsize=None)
def _lrc_case(H, W, field, conf):
    """field "small": disparities in +-3 with negatives (the relu gate); "wide": up to +-W, so samples
    leave the plane on both sides and land in the half-in border cells."""
    d2, d3 = ref.lrc_inputs(B, H, W, 3.0 if field == "small" else float(W), seed=100 * H + W)
    rng = np.random.default_rng(10 * H + W)
    c2, c3 = (rng.uniform(0.0, 1.0, d2.shape).astype(np.float32) if conf else None for _ in range(2))
    g2, g3 = (rng.standard_normal(d2.shape).astype(np.float32) for _ in range(2))
    return d2, d3, c2, c3, g2, g3


@functools.lru_cache(maxsize=None)
def _lrc_reference(H, W, field, conf, use):
    d2, d3, c2, c3, g2, g3 = _lrc_case(H, W, field, conf)
    gs = tuple(x if u else None for x, u in zip((g2, g3), USE[use]))
    return (ref.softlrc_grads(d2, d3, c2, c3, 1.0, *gs, torch.float64),
            ref.softlrc_grads(d2, d3, c2, c3, 1.0, *gs, torch.float32))


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("field", ["small", "wide"])
def test_softlrc_inputs_meet_the_precondition(H, W, field):
    """Every sample point's fractional ix in [0.05, 0.95], |u| >= 1e-3, |d| >= 1e-3, for all pixels of
    both maps; the fields do what they are for."""
    d2, d3 = _lrc_case(H, W, field, False)[:2]
    ok2, ok3 = ref.lrc_precondition(d2, d3)
    assert ok2.all() and ok3.all()
    assert (d2 > 0).any() and (d3 > 0).any()
    # (1, 2) has four pixels a map, and a negative disparity at x = 0 samples at ix = 0 exactly, which the
    # precondition rules out: there one map with a negative entry is what the seed gives
    assert ((d2 < 0).any() and (d3 < 0).any()) if W > 2 else ((d2 < 0).any() or (d3 < 0).any())
    if field == "wide":
        ix2, ix3 = ref.lrc_coords(d2, False)[0], ref.lrc_coords(d3, True)[0]
        assert (np.floor(ix2) == -1).any() and (np.floor(ix3) == W - 1).any()   # the half-in border cells
        if W > 2:   # (|d| <= W = 2 cannot reach past the border cells)
            assert (ix2 < -1).any() and (ix3 > W).any()                   # outside the plane on both sides


@pytest.mark.parametrize("use", list(USE))
@pytest.mark.parametrize("conf", [False, True])
@pytest.mark.parametrize("field", ["small", "wide"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_softlrc_backward(H, W, field, conf, use):
    d2, d3, c2, c3, g2, g3 = _lrc_case(H, W, field, conf)
    want64, want32 = _lrc_reference(H, W, field, conf, use)
    gs = [g(x) if u else None for x, u in zip((g2, g3), USE[use])]
    args = (g(d2), g(d3), g(c2), g(c3), 1.0, *gs, True, True, conf, conf)
    first = ops.softlrc_backward(*args)
    second = ops.softlrc_backward(*args)
    for name, a, b, w64, w32 in zip(("grad_d2", "grad_d3", "grad_conf2", "grad_conf3"), first, second, want64, want32):
        if w64 is None:
            assert a is None and b is None, name
            continue
        assert a.shape == w64.shape and torch.equal(a, b), name + ": two runs differ"
        if np.abs(w64).max() == 0:   # the confidence of the map whose output is not used: written, zero
            assert not c(a).any(), name
            continue
        _check(f"{name} {H}x{W} {field} conf {conf} {use}", c(a), w64, w32)


def test_softlrc_forward_and_partial_requests():
    """ops.softlrc is the kernel of ops.softlrc_joint on separate maps; an output that is not asked for
    is None and the others keep their bits."""
    d2, d3, c2, c3, g2, g3 = _lrc_case(9, 33, "wide", True)
    joint = ops.softlrc_joint(torch.cat([g(d2), g(d3)], 1), torch.cat([g(c2), g(c3)], 1), 1.0)
    s2, s3 = ops.softlrc(g(d2), g(d3), g(c2), g(c3), 1.0)
    assert torch.equal(s2, joint[:, :1]) and torch.equal(s3, joint[:, 1:])
    plain = ops.softlrc_joint(torch.cat([g(d2), g(d3)], 1), None, 1.0)
    s2, s3 = ops.softlrc(g(d2), g(d3))
    assert torch.equal(s2, plain[:, :1]) and torch.equal(s3, plain[:, 1:])
    full = ops.softlrc_backward(g(d2), g(d3), g(c2), g(c3), 1.0, g(g2), g(g3), True, True, True, True)
    for need in ((True, False, False, False), (False, True, False, True), (False, False, True, False)):
        part = ops.softlrc_backward(g(d2), g(d3), g(c2), g(c3), 1.0, g(g2), g(g3), *need)
        for n, a, b in zip(need, part, full):
            assert (a is None) if not n else torch.equal(a, b)


# -------------------------------------------------------------------------------- weighted_lsq
# below one element per thread of the 1024-thread workgroup and below a wave's width times two; below
# one per thread but past a wave; several per thread
SIZES = [70, 594, 4320]
LSQ_USE = {"scale": (1, 0), "shift": (0, 1), "both": (1, 1)}


@functools.lru_cache(maxsize=None)
def _lsq_case(n, kind):
    m, d, cf = ref.lsq_inputs(n, kind)
    rng = np.random.default_rng(n + 1)
    return m, d, cf, rng.standard_normal(2).astype(np.float32), rng.standard_normal(2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _lsq_reference(n, kind, use):
    m, d, cf, gs, gt = _lsq_case(n, kind)
    gs, gt = (x if u else None for x, u in zip((gs, gt), LSQ_USE[use]))
    return (ref.weighted_lsq_grads(m, d, cf, gs, gt, torch.float64),
            ref.weighted_lsq_grads(m, d, cf, gs, gt, torch.float32))


@pytest.mark.parametrize("use", list(LSQ_USE))
@pytest.mark.parametrize("kind", ["random", "zeros", "ties"])
@pytest.mark.parametrize("n", SIZES)
def test_weighted_lsq_backward(n, kind, use):
    m, d, cf, gs, gt = _lsq_case(n, kind)
    want64, want32 = _lsq_reference(n, kind, use)
    tm, td, tc = g(m), g(d), g(cf)
    scale, shift, rec = ops.weighted_lsq_stats(tm, td, tc)
    sc0, sh0 = ops.weighted_lsq(tm, td, tc)
    assert torch.equal(scale, sc0) and torch.equal(shift, sh0)
    assert not c(rec)[:, 5].any()   # full rank
    ups = [g(x) if u else None for x, u in zip((gs, gt), LSQ_USE[use])]
    first = ops.weighted_lsq_backward(tm, td, tc, scale, shift, rec, *ups)
    second = ops.weighted_lsq_backward(tm, td, tc, scale, shift, rec, *ups)
    for name, a, b, w64, w32 in zip(("grad_mde", "grad_disp", "grad_conf"), first, second, want64, want32):
        assert a.shape == w64.shape and torch.equal(a, b), name + ": two runs differ"
        _check(f"{name} n={n} {kind} {use}", c(a), w64, w32)
    if kind == "zeros":
        # the lower threshold is 0 and the zero keys are inside the band: no gradient to disp through
        # the relu, but to mde and conf
        lo, hi = c(rec)[:, 3], c(rec)[:, 4]
        assert (lo == 0).all() and (hi > 0).all()
        zero = d <= 0
        assert zero.mean() > 0.55
        assert not c(first[1])[zero].any()
        assert (c(first[0])[zero] != 0).mean() > 0.99 and (c(first[2])[zero] != 0).mean() > 0.99
    if kind == "ties":
        # membership is <= on both sides: elements equal to a threshold are inside the band
        y, lo, hi = np.maximum(d, 0), c(rec)[:, 3:4].astype(np.float32), c(rec)[:, 4:5].astype(np.float32)
        edge = (y == lo) | (y == hi)
        assert edge.sum() >= 3
        assert (c(first[2])[edge] != 0).all()


def test_weighted_lsq_record_and_partial_requests():
    m, d, cf, gs, gt = _lsq_case(594, "random")
    tm, td, tc = g(m), g(d), g(cf)
    scale, shift, rec = ops.weighted_lsq_stats(tm, td, tc)
    r = c(rec)
    for b in range(2):
        lo, hi, keep = ref.band(torch.from_numpy(d[b]))
        assert r[b, 3] == float(lo) and r[b, 4] == float(hi)
        k = keep.numpy()
        a, wt = np.abs(m[b].astype(np.float64))[k], (0.9 * np.abs(cf[b].astype(np.float64)) + 0.1)[k]
        want = np.array([(wt * a * a).sum(), (wt * a).sum(), wt.sum()])
        assert np.abs(r[b, :3] - want).max() <= 1e-6 * want.max()   # fp32 products, fp64 sums
    full = ops.weighted_lsq_backward(tm, td, tc, scale, shift, rec, g(gs), g(gt))
    for need in ((True, False, False), (False, True, True), (False, False, True)):
        part = ops.weighted_lsq_backward(tm, td, tc, scale, shift, rec, g(gs), g(gt), *need)
        for n, a, b in zip(need, part, full):
            assert (a is None) if not n else torch.equal(a, b)


def test_weighted_lsq_rank_deficient_sample():
    """Sample 0 has all |mde| equal: the forward's minimum-norm branch.  Its gradients are finite and all
    zero; sample 1 is what it is in a batch of its own."""
    m, d, cf, gs, gt = _lsq_case(594, "rank")
    tm, td, tc = g(m), g(d), g(cf)
    scale, shift, rec = ops.weighted_lsq_stats(tm, td, tc)
    sc0, sh0 = ops.weighted_lsq(tm, td, tc)
    assert torch.equal(scale, sc0) and torch.equal(shift, sh0)
    assert c(rec)[:, 5].tolist() == [1.0, 0.0]
    grads = ops.weighted_lsq_backward(tm, td, tc, scale, shift, rec, g(gs), g(gt))
    s1, h1, r1 = ops.weighted_lsq_stats(tm[1:].contiguous(), td[1:].contiguous(), tc[1:].contiguous())
    alone = ops.weighted_lsq_backward(tm[1:].contiguous(), td[1:].contiguous(), tc[1:].contiguous(), s1, h1, r1,
                                      g(gs[1:]), g(gt[1:]))
    for name, a, b in zip(("grad_mde", "grad_disp", "grad_conf"), grads, alone):
        assert torch.isfinite(a).all() and not a[0].any(), name
        assert torch.equal(a[1:], b) and b.any(), name
    # an empty band cannot arise from the quantiles (they are order statistics of the sample); all-zero
    # weights cannot either (0.9 |c| + 0.1 >= 0.1): flag 2 is the kernel's guard only

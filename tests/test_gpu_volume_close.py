"""The hourglass close on the GPU (csrc/volume_close.hip, ops.volume_close_stats / volume_close_backward,
diffops.volume_close) against the float64 reference of tests/volume_close_ref.py: forward mean / rstd
and out, backward dx, dgl and dgr, gated and gate-less, every subset of wanted gradients, a
non-contiguous grad_out and the refusals.

Metric per tensor: max |got - ref64| / max |ref64|.  out, dx, mean and rstd are allowed 4 x the same
metric of torch's fp32 CPU composition on the same inputs (computed here; 2e-7 to 5e-7 for out / dx at
these shapes): the kernels make the same handful of fp32 roundings per cell in another order.  dgl and
dgr are sums of N = D or W products: elementwise (N + 4) 2^-24 mag, mag the same sum over absolute
values.  No cell is left out: the builder keeps every |xh| >= 1e-3 (asserted >= 1e-4), so fp32 and
float64 agree on every LeakyReLU branch."""
import itertools

import pytest
import torch

import volume_close_ref as R
from stereoanywhere_amd import diffops, ops

pytestmark = pytest.mark.gpu

CASES = [(shape, gated) for shape in R.SHAPES for gated in (False, True)]
IDS = [f"{'x'.join(map(str, s))}-{'gated' if g else 'plain'}" for s, g in CASES]


def _gpu(c, *keys):
    return [None if c[k] is None else c[k].cuda() for k in keys]


def _check_metric(name, got, c, key):
    m, allowed = R.metric(got, c["ref"][key]), R.allowance(c, key)
    print(f"{name}: {key} deviates {m:.3g}, allowed {allowed:.3g}")
    assert m <= allowed, (name, key, m, allowed)


def _check_gate(name, got, c, key, terms):
    ref, mag = c["ref"][key], c["mag_l" if key == "dgl" else "mag_r"]
    err = (got.double().cpu() - ref).abs()
    bound = (terms + 4) * R.U * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: {key} uses {worst:.3g} of its ({terms} + 4) u mag bound")
    assert bool((err <= bound).all()), (name, key, worst)


@pytest.mark.parametrize("shape,gated", CASES, ids=IDS)
def test_forward_and_backward(shape, gated):
    c = R.case(shape, gated)
    name = f"{shape} {'gated' if gated else 'plain'}"
    assert float(R.xhat(c["x"]).abs().min()) >= 1e-4
    x, g, gl, gr = _gpu(c, "x", "g", "gl", "gr")
    mean, rstd = ops.volume_close_stats(x, R.EPS)
    _check_metric(name, mean, c, "mean")
    _check_metric(name, rstd, c, "rstd")
    out = diffops.volume_close(x, gl, gr, negative_slope=R.SLOPE, eps=R.EPS)
    _check_metric(name, out, c, "out")
    dx, dgl, dgr = ops.volume_close_backward(g, x, mean, rstd, gl, gr, R.SLOPE, True, gated, gated)
    _check_metric(name, dx, c, "dx")
    if gated:
        _check_gate(name, dgl, c, "dgl", shape[2])
        _check_gate(name, dgr, c, "dgr", shape[4])
    else:
        assert dgl is None and dgr is None


@pytest.mark.parametrize("shape,gated", CASES, ids=IDS)
def test_every_subset_of_wanted_gradients(shape, gated):
    """Through autograd: a wanted gradient is the all-wanted call's, bit for bit; an unwanted one is None."""
    c = R.case(shape, gated)
    x, g, gl, gr = _gpu(c, "x", "g", "gl", "gr")
    mean, rstd = ops.volume_close_stats(x, R.EPS)
    full = ops.volume_close_backward(g, x, mean, rstd, gl, gr, R.SLOPE, True, gated, gated)
    n_in = 3 if gated else 1
    for want in itertools.product((False, True), repeat=n_in):
        ins = [t.clone().requires_grad_(w) for t, w in zip((x, gl, gr), want)]
        out = diffops.volume_close(*ins, negative_slope=R.SLOPE, eps=R.EPS)
        if not any(want):
            assert not out.requires_grad
            continue
        out.backward(g)
        for t, w, ref in zip(ins, want, full):
            assert (t.grad is not None) == w, want
            if w:
                assert torch.equal(t.grad, ref), want


def test_non_contiguous_grad_out():
    shape = R.SHAPES[0]
    c = R.case(shape, True)
    x, gl, gr = (t.requires_grad_(True) for t in _gpu(c, "x", "gl", "gr"))
    out = diffops.volume_close(x, gl, gr)
    g = torch.randn(shape[:2] + (1, 1, 1), generator=torch.Generator().manual_seed(5)).cuda().expand(shape)
    assert not g.is_contiguous()
    out.backward(g)
    ref = R.evaluate(c["x"], g.cpu(), c["gl"], c["gr"], torch.float64)
    f32 = R.evaluate(c["x"], g.cpu(), c["gl"], c["gr"], torch.float32)
    m, allowed = R.metric(x.grad, ref["dx"]), 4.0 * R.metric(f32["dx"], ref["dx"])
    print(f"expanded grad_out: dx deviates {m:.3g}, allowed {allowed:.3g}")
    assert m <= allowed
    mag_l, mag_r = R.gate_mags(c["x"], g.cpu(), c["gl"], c["gr"])
    for got, key, mag, terms in ((gl.grad, "dgl", mag_l, shape[2]), (gr.grad, "dgr", mag_r, shape[4])):
        assert bool(((got.double().cpu() - ref[key]).abs() <= (terms + 4) * R.U * mag).all()), key


def test_refusals():
    x = torch.randn(1, 2, 3, 4, 5, device="cuda")
    gl, gr = torch.rand(1, 2, 4, 5, device="cuda"), torch.rand(1, 2, 4, 3, device="cuda")
    with pytest.raises(ValueError, match="more than one cell"):
        diffops.volume_close(torch.randn(2, 3, 1, 1, 1, device="cuda"))
    with pytest.raises(ValueError, match="both gate maps or neither"):
        diffops.volume_close(x, gl, None)
    with pytest.raises(ValueError, match="both gate maps or neither"):
        diffops.volume_close(x, None, gr)
    with pytest.raises(ValueError, match="gate_left must be"):
        diffops.volume_close(x, gr, gr)
    with pytest.raises(ValueError, match="gate_right must be"):
        diffops.volume_close(x, gl, gl)
    with pytest.raises(ValueError, match="must be \\[B,C,D,H,W\\]"):
        diffops.volume_close(x[0])
    with pytest.raises(RuntimeError, match="on the GPU"):
        diffops.volume_close(x.cpu())
    with pytest.raises(RuntimeError, match="must be float32"):
        ops.volume_close_stats(x.double())
    with pytest.raises(RuntimeError, match="must be contiguous"):
        ops.volume_close_stats(x.transpose(3, 4))
    mean, rstd = ops.volume_close_stats(x)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        ops.volume_close_backward(x.transpose(3, 4), x, mean, rstd)
    with pytest.raises(RuntimeError, match="needs the gate maps"):
        ops.volume_close_backward(x, x, mean, rstd, need_gate_left=True)
    assert diffops.volume_close(x, gl, gr).shape == x.shape   # and the matching call is accepted

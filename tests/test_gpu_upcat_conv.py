"""diffops.upcat_conv and its two backward entry points (csrc/upcat_backward.hip) against the float64 CPU
reference of tests/upcat_conv_ref.py, at the six shapes and both built channel triples, B = 2.

Forward: elementwise within test_gpu_hourglass_ref._upcat_bound (the derived bound of the inference kernel
it is).  Gradients, each tensor on its own: max |got - ref64| / max |ref64| <= 4 x the same metric of torch's
fp32 CPU composition on the same inputs (computed in upcat_conv_ref.case): the op is linear in each argument,
the kernels make the same handful of fp32 roundings per value in another order, so no cell is left out and
there is no kink to keep away from.  Every deviation is printed with its allowance.  Measured on an
MI355X (all 12 cases, seed 0 in each): the forward at 0.02-0.08 of its bound; da at 0.25 of its allowance
(the deviation of torch's own fp32 sum), du 0.12-0.27, dW 0.10-0.43, dp 0.10-0.27."""
import pytest
import torch

import hourglass_ref as HR
import upcat_conv_ref as R
from test_gpu_hourglass_ref import UPCAT_SHAPES, _upcat_bound
from stereoanywhere_amd import diffops, ops

pytestmark = pytest.mark.gpu

assert tuple(UPCAT_SHAPES) == R.SHAPES[:len(UPCAT_SHAPES)]
CASES = [(full, low, triple, lf) for full, low in R.SHAPES for triple, lf in R.TRIPLES]


def _gpu(c, needs=(True, True, True)):
    return [c[k].cuda().requires_grad_(n) for k, n in zip(("skip", "low", "weight"), needs)]


def _report(name, key, got, c):
    m, allowed = R.metric(got, c["ref"][key]), R.allowance(c, key)
    print(f"{name}: {key} deviates {m:.3g}, allowed {allowed:.3g} ({m / allowed:.2f})")
    return m, allowed


@pytest.mark.parametrize("full,low,triple,low_first", CASES, ids=str)
def test_forward(full, low, triple, low_first):
    c = R.case(full, low, triple, low_first)
    ca, cu, _ = triple
    wa, wu = R.split(c["weight"], ca, low_first)
    ref, m = HR.upcat(c["skip"].double(), c["low"].double(), wa, wu)
    assert torch.allclose(ref, c["ref"]["out"], rtol=0, atol=1e-12)
    with torch.no_grad():
        got = diffops.upcat_conv(*_gpu(c, (False,) * 3), low_first)
    assert got.grad_fn is None
    err = (got.double().cpu() - ref).abs()
    bound = _upcat_bound(ca, cu, m)
    print(f"upcat_conv {full} <- {low} {triple}: max err {float(err.max()):.3g}, max err/bound "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3g}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("full,low,triple,low_first", CASES, ids=str)
def test_gradients(full, low, triple, low_first):
    c = R.case(full, low, triple, low_first)
    name = f"upcat_conv {full} <- {low} {triple} seed {c['seed']}"
    skip, lowv, weight = _gpu(c)
    out = diffops.upcat_conv(skip, lowv, weight, low_first)
    out.backward(c["g"].cuda())
    assert weight.grad.shape == c["weight"].shape
    dp = ops.trilinear_up_adjoint(c["g"].cuda(), low)
    worst = [_report(name, key, got, c) for key, got in
             (("da", skip.grad), ("du", lowv.grad), ("dW", weight.grad), ("dp", dp))]
    for m, allowed in worst:
        assert m <= allowed, (name, worst)


@pytest.mark.parametrize("full,low,triple,low_first", [CASES[4], CASES[5], CASES[11]], ids=str)
def test_partial_requests_are_the_full_call_s_bits(full, low, triple, low_first):
    c = R.case(full, low, triple, low_first)
    g = c["g"].cuda()

    def grads(needs):
        t = _gpu(c, needs)
        diffops.upcat_conv(*t, low_first).backward(g)
        return [x.grad for x in t]
    full_call = grads((True, True, True))
    for needs in ((False, True, True), (True, False, False), (False, True, False), (False, False, True),
                  (True, True, False), (True, False, True)):
        got = grads(needs)
        for k, (need, a, b) in enumerate(zip(needs, got, full_call)):
            assert (a is not None) == need, (needs, k)
            if need:
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (needs, k)


@pytest.mark.parametrize("triple,low_first", R.TRIPLES, ids=str)
def test_saves_exactly_skip_low_and_weight(triple, low_first):
    full, low = R.SHAPES[0]
    c = R.case(full, low, triple, low_first)
    skip, lowv, weight = _gpu(c)
    packed = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(t) or t, lambda t: t):
        out = diffops.upcat_conv(skip, lowv, weight, low_first)
    assert sorted(t.data_ptr() for t in packed) == sorted(t.data_ptr() for t in (skip, lowv, weight))
    assert sorted(tuple(t.shape) for t in packed) == sorted(tuple(t.shape) for t in (skip, lowv, weight))
    out.sum().backward()


def test_refusals():
    c = R.case(*R.SHAPES[3], *R.TRIPLES[0])
    skip, lowv, weight = _gpu(c, (False,) * 3)
    with pytest.raises(ValueError, match=r"built for \(Ca, Cu, Cout\) in \(\(8, 16, 8\), \(16, 32, 16\)\)"):
        diffops.upcat_conv(skip[:, :4].contiguous(), lowv, weight[:, :20].contiguous(), False)
    with pytest.raises(ValueError, match="at most half size"):
        diffops.upcat_conv(skip, torch.zeros(2, 16, 2, 1, 1, device="cuda"), weight, False)
    with pytest.raises(ValueError, match="D, H and W must be at least 2"):
        diffops.upcat_conv(skip[:, :, :1].contiguous(), lowv, weight, False)
    with pytest.raises(ValueError, match=r"weight must be \[Cout, Ca \+ Cu = 24, 1, 1, 1\]"):
        diffops.upcat_conv(skip, lowv, weight[:, :23].contiguous(), False)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        diffops.upcat_conv(skip.cpu(), lowv, weight, False)
    with pytest.raises(RuntimeError, match="no kernel built for 8 x 16"):
        ops.conv3d_pointwise_backward(skip, torch.zeros(2, 16, 2, 2, 2, device="cuda"), torch.zeros(8, 16, device="cuda"))

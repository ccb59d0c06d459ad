"""The HIP adjoints of soft-argmin / entropy confidence and of convex up-sampling
(csrc/diffops_backward.hip) through ops.softargmin_conf_backward / ops.convex_upsample_backward,
against torch.autograd of the reference formulation in float64 (tests/diffops_ref.py) from the same
fp32 inputs.

The yardstick is the reference formulation's own fp32 autograd on the CPU: with
e_ref = max |grad_fp32_torch - grad_fp64|, each gradient tensor must satisfy
max |grad_hip - grad_fp64| <= 4 e_ref (the 4 covers a different but fixed summation order, the
recomputed softmax and the device's exp / log2).  Every case is run twice: the two results must be
the same bits."""
import functools

import numpy as np
import pytest
import torch

import diffops_ref as ref
from stereoanywhere_amd import ops

pytestmark = pytest.mark.gpu
dev = "cuda"


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


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


# ------------------------------------------------------------------------------- soft-argmin
# (300 is past every 256 / 288 boundary of the forward's dispatch and takes the backward's re-reading
# paths; (256, 257): the last size of the register-resident paths on one axis, the first past it on
# the other, in either layout; (5, 6): a strided line shorter than the 4 segments the statistics
# kernel's waves split it into at whole strides)
SHAPES = [(44, 44), (37, 50), (64, 64), (300, 300), (256, 257), (5, 6)]
CASES = {"all": (1, 1, 1, 1), "dL": (1, 0, 0, 0), "cR": (0, 0, 0, 1), "conf": (0, 0, 1, 1)}
B, H = 2, 3


@functools.lru_cache(maxsize=None)
def _sam_inputs(W1, W2, scale):
    rng = np.random.default_rng(100 * W1 + W2 + int(scale))
    vols = []
    for _ in range(2):
        v = (scale * rng.standard_normal((B, H, W1, W2))).astype(np.float32)
        v[0, 1, 2, :] = v[0, 1, 2, 0]    # a constant row: uniform softmax over k
        v[1, 2, 3, 1] = v[1, 2].max() + 60.0    # one logit 60 above the rest: p -> 1 on both sides
        vols.append(v)
    grads = [rng.standard_normal((B, H, n)).astype(np.float32) for n in (W1, W2, W1, W2)]
    return vols, grads


@functools.lru_cache(maxsize=None)
def _sam_reference(W1, W2, scale, case):
    (vd, vc), grads = _sam_inputs(W1, W2, scale)
    gs = tuple(x if u else None for x, u in zip(grads, CASES[case]))
    return ref.softargmin_grads(vd, vc, gs, torch.float64), ref.softargmin_grads(vd, vc, gs, torch.float32)


def _device_volume(v, layout):
    """(tensor viewed [B,H,W1,W2], strides (sb, sh, sj, sk)) in the reference layout (k contiguous) or
    the native one (storage [B,W2,H,W1]: j contiguous)."""
    t = g(v)
    if layout == "native":
        t = t.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    return t, tuple(t.stride())


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("scale", [4.0, 30.0])
@pytest.mark.parametrize("layout", ["reference", "native"])
@pytest.mark.parametrize("W1,W2", SHAPES)
def test_softargmin_backward(W1, W2, layout, scale, case):
    (vd, vc), grads = _sam_inputs(W1, W2, scale)
    want64, want32 = _sam_reference(W1, W2, scale, case)
    use = CASES[case]
    td, strides = _device_volume(vd, layout)
    tc, _ = _device_volume(vc, layout)
    gs = [g(x) if u else None for x, u in zip(grads, use)]
    runs = []
    for _ in range(2):
        od = torch.full_like(td, float("nan"))
        oc = torch.full_like(tc, float("nan"))
        assert od.stride() == td.stride()
        ops.softargmin_conf_backward(td if use[0] or use[1] else None, tc, strides, (B, H, W1, W2), *gs,
                                     out_disp=od, out_conf=oc)
        runs.append((c(od), c(oc)))
    for name, a, b, w64, w32 in zip(("grad_vol_disp", "grad_vol_conf"), runs[0], runs[1], want64, want32):
        assert np.array_equal(a, b, equal_nan=True), name + ": two runs differ"
        if w64 is None:   # no upstream gradient: the buffer is not touched
            assert np.isnan(a).all(), name
        else:
            _check(f"{name} {W1}x{W2} {layout} scale {scale:g} {case}", a, w64, w32)


@pytest.mark.parametrize("layout", ["reference", "native"])
def test_softargmin_backward_without_workspace(layout):
    """The workspace holds the strided side's statistics only: with gradients on the contiguous side
    alone (the left maps in the reference layout, the right ones in the native layout) the call takes
    a null workspace and gives the bits of the call through ops."""
    from stereoanywhere_amd import _native as N
    W1, W2, scale = 37, 50, 4.0
    (vd, vc), grads = _sam_inputs(W1, W2, scale)
    td, strides = _device_volume(vd, layout)
    tc, _ = _device_volume(vc, layout)
    use = (1, 0, 1, 0) if layout == "reference" else (0, 1, 0, 1)
    gs = [g(x) if u else None for x, u in zip(grads, use)]
    want = ops.softargmin_conf_backward(td, tc, strides, (B, H, W1, W2), *gs)
    od, oc = torch.full_like(td, float("nan")), torch.full_like(tc, float("nan"))
    p = [None if t is None else t.data_ptr() for t in gs]
    N.call("sa_softargmin_conf_backward", td.data_ptr(), tc.data_ptr(), B, H, W1, W2, *strides, *p, od.data_ptr(),
           oc.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(od, want[0]) and torch.equal(oc, want[1])


# ------------------------------------------------------------------------- convex up-sampling
GEOS = [(1, 1, 4), (5, 7, 4), (9, 33, 4), (5, 7, 2), (5, 7, 8), (5, 7, 1)]


@functools.lru_cache(maxsize=None)
def _cub_inputs(Hc, Wc, f, mscale):
    rng = np.random.default_rng(1000 * Hc + 10 * Wc + f + int(mscale))
    flow = (10.0 * rng.standard_normal((2, 1, Hc, Wc))).astype(np.float32)
    mask = (mscale * rng.standard_normal((2, 9 * f * f, Hc, Wc))).astype(np.float32)
    gout = rng.standard_normal((2, 1, f * Hc, f * Wc)).astype(np.float32)
    return flow, mask, gout


@functools.lru_cache(maxsize=None)
def _cub_reference(Hc, Wc, f, mscale, use_scale):
    flow, mask, gout = _cub_inputs(Hc, Wc, f, mscale)
    return (ref.convex_grads(flow, mask, gout, f, use_scale, torch.float64),
            ref.convex_grads(flow, mask, gout, f, use_scale, torch.float32))


@pytest.mark.parametrize("need", ["flow", "mask", "both"])
@pytest.mark.parametrize("use_scale", [True, False])
@pytest.mark.parametrize("mscale", [1.0, 8.0])
@pytest.mark.parametrize("Hc,Wc,f", GEOS)
def test_convex_upsample_backward(Hc, Wc, f, mscale, use_scale, need):
    flow, mask, gout = _cub_inputs(Hc, Wc, f, mscale)
    want64, want32 = _cub_reference(Hc, Wc, f, mscale, use_scale)
    need_flow, need_mask = need != "mask", need != "flow"
    # the mask as a channel slice of a wider buffer: a batch stride that is not its size
    wide = torch.zeros((2, 9 * f * f + 3, Hc, Wc), device=dev)
    wide[:, :9 * f * f] = g(mask)
    args = (g(flow), wide[:, :9 * f * f], g(gout), f, float(f) if use_scale else 1.0, need_flow, need_mask)
    first = ops.convex_upsample_backward(*args)
    second = ops.convex_upsample_backward(*args)
    for name, a, b, w64, w32, needed in zip(("grad_flow", "grad_mask"), first, second, want64, want32,
                                            (need_flow, need_mask)):
        if not needed:
            assert a is None and b is None, name
            continue
        assert a.shape == w64.shape and torch.equal(a, b), name + ": two runs differ"
        _check(f"{name} {Hc}x{Wc} f{f} mask scale {mscale:g} use_scale {use_scale} {need}", c(a), w64, w32)

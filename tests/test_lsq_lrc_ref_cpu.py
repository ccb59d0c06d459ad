"""The closed-form gradients that csrc/lsq_backward.hip implements (tests/lsq_lrc_ref.py, numpy
float64) against torch.autograd of the reference formulation in float64 on the CPU, the restated
forwards against oracle/ops_ref.py, and the argument errors of the new ops wrappers (raised before any
device call: this file runs without a GPU)."""
import numpy as np
import pytest
import torch

import lsq_lrc_ref as ref
from oracle import ops_ref as R
from stereoanywhere_amd import ops


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ------------------------------------------------------------------------------------ forwards
@pytest.mark.parametrize("H,W,amp", [(1, 2, 3.0), (5, 7, 3.0), (5, 7, 7.0), (9, 33, 33.0)])
def test_softlrc_restatement_matches_oracle(H, W, amp):
    """fp32 against fp32: the same formula, the divisions and the blend in another order (a few ulp of
    values up to 1, coordinates up to 2 W)."""
    d2, d3 = ref.lrc_inputs(2, H, W, amp, seed=3)
    s2, s3 = ref.softlrc(torch.from_numpy(d2), torch.from_numpy(d3))
    o2, o3 = R.softlrc(d2, d3, 1.0)
    for name, a, b in (("s2", s2.numpy(), o2), ("s3", s3.numpy(), o3)):
        print(f"{name} {H}x{W}: max difference {np.abs(a - b).max():.3g}")
        assert a.shape == b.shape and np.abs(a - b).max() <= 2e-5 * max(1.0, W / 8), name
    # and the float64 closed form's forward against the float64 restatement
    (c2, c3), _ = ref.closed_softlrc(d2, d3, None, None, 1.0, None, None)
    t2, t3 = ref.softlrc(torch.from_numpy(d2).double(), torch.from_numpy(d3).double())
    assert np.abs(c2 - t2.numpy()).max() <= 1e-12 and np.abs(c3 - t3.numpy()).max() <= 1e-12


@pytest.mark.parametrize("n", [70, 594])
def test_weighted_lsq_restatement_matches_oracle(n):
    m, d, c = ref.lsq_inputs(n, "random")
    want = R.weighted_lsq(m, d, c)
    got = ref.weighted_lsq(*(torch.from_numpy(a) for a in (m, d, c)), torch.float64)
    (cs, ct), _ = ref.closed_weighted_lsq(m, d, c, None, None)
    for name, a, b, cl in zip(("scale", "shift"), got, want, (cs, ct)):
        # the oracle rounds the products a w, w, y w to fp32 before its float64 solve and its result to fp32
        assert np.abs(a.numpy() - b).max() <= 1e-5 * max(1.0, np.abs(b).max()), name
        assert np.abs(a.numpy() - cl).max() <= 1e-12 * max(1.0, np.abs(cl).max()), name


# ------------------------------------------------------------------------------------ adjoints
@pytest.mark.parametrize("H,W,amp", [(1, 2, 3.0), (5, 7, 3.0), (5, 7, 7.0), (4, 19, 19.0)])
@pytest.mark.parametrize("conf", [False, True])
@pytest.mark.parametrize("use", [(1, 0), (0, 1), (1, 1)])
def test_softlrc_closed_form_matches_autograd(H, W, amp, conf, use):
    """max |a - b| / max |b| <= 1e-12: both sides are float64 sums of a few terms."""
    d2, d3 = ref.lrc_inputs(2, H, W, amp, seed=5)
    rng = np.random.default_rng(7)
    c2, c3 = (rng.uniform(-0.2, 1.0, d2.shape) if conf else None for _ in range(2))
    g2, g3 = (rng.standard_normal(d2.shape) if u else None for u in use)
    want = ref.softlrc_grads(d2, d3, c2, c3, 1.0, g2, g3, torch.float64)
    _, got = ref.closed_softlrc(d2, d3, c2, c3, 1.0, g2, g3)
    for name, a, b in zip(("grad_d2", "grad_d3", "grad_conf2", "grad_conf3"), got, want):
        assert (a is None) == (b is None), name
        if b is None:
            continue
        if np.abs(b).max() == 0:   # the confidence of the map whose output is not used
            assert np.abs(a).max() == 0, name
            continue
        print(f"{name}: relative difference {_rel(a, b):.3g}")
        assert a.shape == b.shape and _rel(a, b) <= 1e-12, name


@pytest.mark.parametrize("n", [70, 594, 1360])
@pytest.mark.parametrize("kind", ["random", "zeros", "ties"])
@pytest.mark.parametrize("use", [(1, 0), (0, 1), (1, 1)])
def test_weighted_lsq_closed_form_matches_autograd(n, kind, use):
    m, d, c = ref.lsq_inputs(n, kind)
    rng = np.random.default_rng(11)
    gs, gt = (rng.standard_normal(2) if u else None for u in use)
    want = ref.weighted_lsq_grads(m, d, c, gs, gt, torch.float64)
    _, got = ref.closed_weighted_lsq(m, d, c, gs, gt)
    for name, a, b in zip(("grad_mde", "grad_disp", "grad_conf"), got, want):
        print(f"{name} n={n} {kind}: relative difference {_rel(a, b):.3g}")
        assert a.shape == b.shape and _rel(a, b) <= 1e-12, name
        assert np.abs(b).max() > 0


# ------------------------------------------------------------------------ wrapper argument errors
class _Fake(torch.Tensor):
    """A CPU tensor that reports itself on the GPU: it passes the wrappers' device check, so their
    shape / contiguity / nothing-to-compute errors can be reached without a device.  Any kernel launch
    would dereference a host pointer; none is reached."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def device(self):
        return torch.device("cuda", 0)


def _f(*shape, dtype=torch.float32):
    return _Fake(torch.zeros(shape, dtype=dtype))


def test_softlrc_wrapper_errors():
    d = torch.zeros(2, 1, 3, 4)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        ops.softlrc(d, d)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        ops.softlrc_backward(d, d, None, None, 1.0, d, d)
    a = _f(2, 1, 3, 4)
    with pytest.raises(RuntimeError, match=r"d2 must be \[B,1,H,W\]"):
        ops.softlrc(_f(2, 2, 3, 4), _f(2, 2, 3, 4))
    with pytest.raises(RuntimeError, match="d3 must have d2's shape"):
        ops.softlrc(a, _f(2, 1, 3, 5))
    with pytest.raises(RuntimeError, match="conf3 must have d2's shape"):
        ops.softlrc_backward(a, a, a, _f(2, 1, 4, 4), 1.0, a, a)
    with pytest.raises(RuntimeError, match="must be float32"):
        ops.softlrc(a, _f(2, 1, 3, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="d3 must be contiguous"):
        ops.softlrc(a, _Fake(torch.zeros(2, 1, 4, 3).transpose(2, 3)))
    with pytest.raises(RuntimeError, match="g_s3 must have d2's shape"):
        ops.softlrc_backward(a, a, None, None, 1.0, a, _f(2, 1, 3, 3))
    with pytest.raises(RuntimeError, match="without that confidence"):
        ops.softlrc_backward(a, a, None, a, 1.0, a, a, need_conf2=True)
    with pytest.raises(RuntimeError, match="nothing to compute"):
        ops.softlrc_backward(a, a, a, a, 1.0, a, a, need_d2=False, need_d3=False)
    with pytest.raises(RuntimeError, match="nothing to compute"):
        ops.softlrc_backward(a, a, a, a, 1.0, None, None)


def test_weighted_lsq_wrapper_errors():
    m = torch.zeros(2, 70)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        ops.weighted_lsq_stats(m, m, m)
    a, s = _f(2, 70), _f(2)
    rec = _f(2, ops.LSQ_REC, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        ops.weighted_lsq_backward(m, m, m, s, s, rec, s, s)
    with pytest.raises(RuntimeError, match="conf must have mde's shape"):
        ops.weighted_lsq_stats(a, a, _f(2, 71))
    with pytest.raises(RuntimeError, match=r"must be \[B, ...\] and not empty"):
        ops.weighted_lsq_stats(_f(70), _f(70), _f(70))
    with pytest.raises(RuntimeError, match="disp must be contiguous"):
        ops.weighted_lsq_stats(a, _Fake(torch.zeros(70, 2).t()), a)
    with pytest.raises(RuntimeError, match="scale must hold B = 2 floats"):
        ops.weighted_lsq_backward(a, a, a, _f(3), s, rec, s, s)
    with pytest.raises(RuntimeError, match="g_shift must hold B = 2 floats"):
        ops.weighted_lsq_backward(a, a, a, s, s, rec, s, _f(1))
    for bad in (_f(2, ops.LSQ_REC), _f(2, 5, dtype=torch.float64), torch.zeros(2, ops.LSQ_REC, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="rec must be the contiguous float64"):
            ops.weighted_lsq_backward(a, a, a, s, s, bad, s, s)
    with pytest.raises(RuntimeError, match="nothing to compute"):
        ops.weighted_lsq_backward(a, a, a, s, s, rec, s, s, need_mde=False, need_disp=False, need_conf=False)
    with pytest.raises(RuntimeError, match="nothing to compute"):
        ops.weighted_lsq_backward(a, a, a, s, s, rec, None, None)


def test_native_refusals():
    """The entry points' own refusals: SA_E_ARG and a message that names the limit, before any HIP call."""
    from stereoanywhere_amd import _native as N
    lib, P = N.lib(), 64
    assert lib.sa_softlrc_backward_ws_size(4, 136, 240) == 4 * 8 * 4 * 136 * 240
    assert lib.sa_softlrc_backward_ws_size(0, 3, 4) == -1

    def lrc(d2=P, conf2=P, g=(P, P), outs=(P, P, P, P), ws=P, H=3, bs=12):
        return lib.sa_softlrc_backward(d2, P, conf2, P, 1, H, 4, bs, 1.0, *g, *outs, ws, None)

    for kw, msg in (({"d2": None}, b"null pointer (d2 / d3)"), ({"g": (None, None)}, b"both upstream gradients"),
                    ({"outs": (None,) * 4}, b"all four outputs"), ({"conf2": None}, b"grad_conf2 requested without conf2"),
                    ({"H": 0}, b"empty shape"), ({"bs": 11}, b"map_bs too small"), ({"ws": None}, b"null pointer (workspace"),
                    ({"ws": P + 4}, b"8-byte aligned")):
        assert lrc(**kw) == -1 and msg in lib.sa_last_error(), kw

    def stats(rec=P, n=70, q=(0.2, 0.9)):
        return lib.sa_weighted_lsq_stats(P, P, P, 2, n, *q, P, P, rec, None)

    for kw, msg in (({"rec": None}, b"null pointer"), ({"n": 0}, b"empty input"), ({"q": (0.9, 0.2)}, b"quantiles out of order"),
                    ({"rec": P + 4}, b"8-byte aligned")):
        assert stats(**kw) == -1 and b"sa_weighted_lsq_stats" in lib.sa_last_error() and msg in lib.sa_last_error(), kw

    def bwd(rec=P, g=(P, P), outs=(P, P, P), B=2):
        return lib.sa_weighted_lsq_backward(P, P, P, B, 70, P, P, rec, *g, *outs, None)

    for kw, msg in (({"rec": None}, b"null pointer"), ({"g": (None, None)}, b"both upstream gradients"),
                    ({"outs": (None,) * 3}, b"all three outputs"), ({"B": 0}, b"empty input"), ({"rec": P + 4}, b"8-byte aligned")):
        assert bwd(**kw) == -1 and b"sa_weighted_lsq_backward" in lib.sa_last_error() and msg in lib.sa_last_error(), kw

"""The fused lookup + convc1 (ops.corr_lookup_conv1x1 and its sheared form) at pyramid geometries
other than the published 4 levels of radius 4: 1..4 levels, radius 1..8 (csrc/lookup_fold.h)."""
import numpy as np
import pytest
import torch

from fixtures_util import load_fixture
from stereoanywhere_amd import _native as N, ops

pytestmark = pytest.mark.gpu
dev = "cuda"

GEOMETRIES = [(1, 1), (2, 3), (3, 2), (4, 1), (4, 5), (4, 8), (1, 8)]


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def c(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _coords(rng, B, H, W, R):
    """[B,1,H,W] covering [-R-3, W+R+3]: every integer and every .5 of the range among them."""
    lo, hi = -R - 3, W + R + 3
    n = B * H * W
    exact = np.arange(lo, hi + 0.25, 0.5, dtype=np.float32)
    assert exact.size < n
    cx = np.concatenate([exact, (rng.random(n - exact.size) * (hi - lo) + lo).astype(np.float32)])
    rng.shuffle(cx)
    return cx.reshape(B, 1, H, W)


def _case(L, R, B, H, W, seed):
    rng = np.random.default_rng(seed)
    va, vb = (g(rng.standard_normal((B, H, W, W))) for _ in range(2))
    NT = L * (2 * R + 1)
    wt = (rng.standard_normal((NT, 64)) / np.sqrt(NT)).astype(np.float32)
    bias = rng.standard_normal(64).astype(np.float32)
    return (ops.pyramid_from_volume(va, L), ops.pyramid_from_volume(vb, L), _coords(rng, B, H, W, R), wt, bias)


@pytest.mark.parametrize("L,R", GEOMETRIES)
def test_fused_vs_unfused(L, R):
    """Against ops.corr_lookup followed by the 1x1 conv + bias + ReLU in float64 on the host.
    Per element |got - ref| <= (NT + 2) 2^-24 (|b_c| + sum_k |w_kc tap_k|), NT = L (2R + 1): the
    forward error bound of the NT-long fp32 fmaf chain the kernel is specified to run (each step
    rounds once, relative 2^-24), plus the final rounding of the float64 reference to compare;
    ReLU does not grow a difference.  Level widths 44, 22, 11, 5; 440 pixels (no multiple of 64)."""
    B, H, W = 2, 5, 44
    pa, pb, cx, wt, bias = _case(L, R, B, H, W, 100 * L + R)
    NT = L * (2 * R + 1)
    got = c(ops.corr_lookup_conv1x1(pa, pb, W, L, R, g(cx), g(wt), g(bias))).astype(np.float64)
    taps = c(ops.corr_lookup(pa, pb, W, L, R, g(cx))).astype(np.float64)      # [B, 2 NT, H, W]
    w64, b64 = wt.astype(np.float64), bias.astype(np.float64)
    for v in range(2):
        t = taps[:, NT * v:NT * (v + 1)]
        ref = np.maximum(np.einsum("kc,bkhw->bchw", w64, t) + b64[None, :, None, None], 0)
        mag = np.einsum("kc,bkhw->bchw", np.abs(w64), np.abs(t)) + np.abs(b64)[None, :, None, None]
        err = np.abs(got[v::2] - ref)
        bound = (NT + 2) * 2.0 ** -24 * mag
        print(f"L={L} R={R} vol {v}: max err {err.max():.3g}, max err/bound {(err / bound).max():.3g}")
        assert np.all(err <= bound)
        assert np.any(ref > 0) and np.any(ref == 0)


@pytest.mark.parametrize("two", [True, False])
@pytest.mark.parametrize("L,R", GEOMETRIES)
def test_sheared_equals_row_layout(L, R, two):
    """The sheared kernel and the row-layout kernel run one device function on the same cells:
    the same bits, with and without the second pyramid."""
    B, H, W = 1, 6, 48
    assert ops.shear_supported(B, H, W, W, L)
    pa, pb, cx, wt, bias = _case(L, R, B, H, W, 7 * L + R)
    if not two:
        pb = None
    row = ops.corr_lookup_conv1x1(pa, pb, W, L, R, g(cx), g(wt), g(bias))
    sa = ops.corr_pyramid_shear(pa, B, H, W, W, L)
    sb = None if pb is None else ops.corr_pyramid_shear(pb, B, H, W, W, L)
    sh = ops.corr_lookup_conv1x1_sheared(sa, sb, W, L, R, g(cx), g(wt), g(bias))
    torch.cuda.synchronize()
    assert row.shape == (B * (2 if two else 1), 64, H, W)
    assert torch.equal(row, sh)
    assert bool((row > 0).any())


def test_published_geometry_untouched():
    """(4, 4) beside the new dispatch: the fused op against the reference's own lookup vector.
    Identity convc1 weights of either sign give relu(tap) and relu(-tap) exactly."""
    micro = load_fixture("micro_ops.npz")
    vol = micro["corr.out"][:, :, :, 0]  # [2,3,37,45]
    W2 = vol.shape[-1]
    pyr = ops.pyramid_from_volume(g(vol), 4)
    cx = g(micro["lookup.coords"])[:, :1].contiguous()
    eye = np.zeros((36, 64), np.float32)
    eye[np.arange(36), np.arange(36)] = 1.0
    zero = g(np.zeros(64, np.float32))
    pos = c(ops.corr_lookup_conv1x1(pyr, None, W2, 4, 4, cx, g(eye), zero))
    neg = c(ops.corr_lookup_conv1x1(pyr, None, W2, 4, 4, cx, g(-eye), zero))
    np.testing.assert_allclose(pos[:, :36] - neg[:, :36], micro["lookup.out"], atol=1e-5)
    assert np.all(pos[:, 36:] == 0)


def test_out_of_range_raises():
    rng = np.random.default_rng(0)
    B, H, W = 1, 2, 48
    pyr = ops.pyramid_from_volume(g(rng.standard_normal((B, H, W, W))), 4)
    cx = g(rng.random((B, 1, H, W)) * W)
    bias = g(np.zeros(64, np.float32))

    def run(p, W2, L, R):
        return ops.corr_lookup_conv1x1(p, None, W2, L, R, cx, g(np.zeros((L * (2 * R + 1), 64), np.float32)), bias)
    with pytest.raises(N.NativeError, match=r"1\.\.4 levels, radius 1\.\.8"):
        run(pyr, W, 5, 4)
    with pytest.raises(N.NativeError, match=r"1\.\.4 levels, radius 1\.\.8"):
        run(pyr, W, 4, 9)
    # widths 8, 4, 2, 1: the last level cannot be sampled
    narrow = ops.pyramid_from_volume(g(rng.standard_normal((B, H, W, 8))), 4)
    with pytest.raises(N.NativeError, match="too narrow"):
        run(narrow, 8, 4, 2)
    sh = ops.corr_pyramid_shear(pyr, B, H, W, W, 4)
    with pytest.raises(N.NativeError, match=r"1\.\.4 levels, radius 1\.\.8"):
        ops.corr_lookup_conv1x1_sheared(sh, None, W, 4, 9, cx, g(np.zeros((4 * 19, 64), np.float32)), bias)

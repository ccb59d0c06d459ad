"""The split F(4x4,3x3) kernel (conv2d_wino4.hip, W4Split) after two changes to its VALU work: the
operand split of a lane's two channels in 5 instructions against the filter image ordered
[hi | lo][job] (w4_pair_split, wino4s_weights_kernel), and the 2^-12 (and range-guard) rescale
folded into the epilogue's finishing FMA.  Smallest shapes that reach every path the changes
touch: one and two 8-channel chunks, one whole 8 x 128 block, ragged right and bottom edges of a
16 x 64 block (12 x 20), several blocks in both directions (20 x 132: a tie between the two
geometries, which goes to 16 x 64 blocks, 3 x 2 of them) and two 8 x 128 blocks across with a ragged
edge (8 x 132); bias + ReLU, the mode-1 and mode-2 gate epilogues, an affine-input launch, the range
guard's second pass.  Reference: float64 conv2d.  Tolerance: test_gpu_wino.py's for the split
kernel (1e-4 max, 1e-5 RMS of the output's RMS, floor 1)."""
import pytest
import torch
import torch.nn.functional as F

from stereoanywhere_amd import ops

pytestmark = pytest.mark.gpu
dev = "cuda"


def rnd(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev)


def _run(monkeypatch, *probs):
    monkeypatch.setattr(ops, "_WINO4", True)
    monkeypatch.setattr(ops, "W4_SPLIT", True)
    monkeypatch.setattr(ops, "_WINO4_MIN_BLOCKS", 0)   # small test shapes still take the F(4x4) path
    ops.WORK = {}
    ops.W4_SHAPE_LAUNCHES.clear()
    try:
        res = ops.conv2d_k3_multi(*probs)
        work = dict(ops.WORK)
    finally:
        ops.WORK = None
    assert "conv2d_wino4" in work and "conv2d_wino" not in work
    assert set(ops.W4_SHAPE_LAUNCHES) == {6}, ops.W4_SHAPE_LAUNCHES   # the split kernel
    return res


def _filters(monkeypatch, w):
    monkeypatch.setattr(ops, "W4_SPLIT", True)
    U = ops.wino_weights(w)
    assert U.u4s is not None
    return U


def _redo_blocks():
    from stereoanywhere_amd import _native as N
    n = int(N.lib().sa_split_redo_blocks(1))
    assert n >= 0
    return n


def _check(got, ref64, what):
    ref = ref64.float()
    scale = max(float(ref.pow(2).mean().sqrt()), 1.0)
    err_max, err_rms = float((got - ref).abs().max()), float((got - ref).pow(2).mean().sqrt())
    print(f"split5 {what}: max {err_max:.2e} rms {err_rms:.2e} (scale {scale:.2f})")
    assert err_max < 1e-4 * scale and err_rms < 1e-5 * scale, (what, err_max, err_rms)


@pytest.mark.parametrize("Cin", [8, 16])
@pytest.mark.parametrize("H,W", [(8, 128), (12, 20), (20, 132), (8, 132)])
def test_split5_matches_conv2d(monkeypatch, Cin, H, W):
    x = rnd(1, Cin, H, W, seed=Cin + H)
    w = rnd(32, Cin, 3, 3, seed=W) / (3 * Cin ** 0.5)
    b = rnd(32, seed=8)
    U = _filters(monkeypatch, w)
    for bias, relu in ((None, False), (b, True)):
        (got,) = _run(monkeypatch, dict(x=x, U=U, bias=bias, relu=relu))
        ref = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), padding=1)
        _check(got, torch.relu(ref) if relu else ref, f"{Cin}->32 {H}x{W} bias/relu {relu}")


def test_split5_gate_epilogues(monkeypatch):
    """Modes 1 and 2 at 8 x 128, built as test_gpu_wino.py::test_wino4_gru_gate_epilogues builds them
    (mode 1 needs whole 32-channel blocks of z and of r: 32 hidden channels), against float64."""
    g = torch.Generator(device="cpu").manual_seed(42)

    def r(*s):
        return torch.randn(*s, generator=g).to(dev)
    B, hd, xd, H, W = 1, 32, 16, 8, 128
    hxr = r(B, 2 * hd + xd, H, W)
    h, x, rh_out = hxr[:, :hd], hxr[:, hd:hd + xd], hxr[:, hd + xd:]
    ctx = r(B, 3 * hd, H, W)
    wz, wr, wq = (r(hd, hd + xd, 3, 3) / (3 * (hd + xd) ** 0.5) for _ in range(3))
    bz, br, bq = r(hd), r(hd), r(hd)
    z = torch.empty(B, hd, H, W, device=dev)
    qx = torch.empty(B, hd, H, W, device=dev)
    d = torch.Tensor.double
    hx = torch.cat([h, x], 1).clone()
    h0 = h.clone()
    zo, qxo = _run(monkeypatch,
                   dict(x=hxr[:, :hd + xd], U=_filters(monkeypatch, torch.cat([wz, wr]).contiguous()),
                        bias=torch.cat([bz, br]), out=z, gate=dict(mode=1, ctx=ctx, h=h, out2=rh_out)),
                   dict(x=x, U=_filters(monkeypatch, wq[:, hd:].contiguous()), out=qx))
    assert zo is z and qxo is qx
    z_ref = torch.sigmoid(F.conv2d(d(hx), d(wz), d(bz), padding=1) + d(ctx[:, :hd]))
    r_ref = torch.sigmoid(F.conv2d(d(hx), d(wr), d(br), padding=1) + d(ctx[:, hd:2 * hd]))
    # (test_wino4_gru_gate_epilogues' tolerances)
    torch.testing.assert_close(z, z_ref.float(), atol=3e-5, rtol=1e-4)
    torch.testing.assert_close(rh_out, (r_ref * d(h0)).float(), atol=3e-5, rtol=1e-4)
    torch.testing.assert_close(qx, F.conv2d(d(x), d(wq[:, hd:]), padding=1).float(), atol=1e-4, rtol=1e-4)
    # mode 2: h <- (1 - z) h + z tanh(convq(cat(r*h, x)) + cq), the x part given as the addend, in place
    q_ref = torch.tanh(F.conv2d(torch.cat([d(rh_out), d(x)], 1), d(wq), d(bq), padding=1) + d(ctx[:, 2 * hd:]))
    h_ref = ((1 - d(z)) * d(h0) + d(z) * q_ref).float()
    (ho,) = _run(monkeypatch, dict(x=rh_out, U=_filters(monkeypatch, wq[:, :hd].contiguous()), bias=bq, out=h,
                                   gate=dict(mode=2, ctx=ctx[:, 2 * hd:], h=h, z=z, add=qx)))
    assert ho is h
    torch.testing.assert_close(h, h_ref, atol=1e-4, rtol=1e-4)


def test_split5_affine_input(monkeypatch):
    """The affine-input instance (the paired loop with the producer's scale, shift and ReLU applied
    on load): two chunks, ragged 16 x 64 blocks."""
    x = rnd(1, 16, 12, 20, seed=5)
    w = rnd(32, 16, 3, 3, seed=6) / 12
    s, t = rnd(16, seed=9).abs() + 0.5, rnd(16, seed=10)
    (got,) = _run(monkeypatch, dict(x=x, U=_filters(monkeypatch, w), in_aff=ops.Affine(None, s, t), in_act="relu"))
    xin = torch.relu(x.double() * s.double()[:, None, None] + t.double()[:, None, None])
    _check(got, F.conv2d(xin, w.double(), padding=1), "affine input 16->32 12x20")


def test_split5_range_guard(monkeypatch):
    """Input magnitude 3e3 (where test_wino4_split_range_guard sees the guard firing): the block runs
    again on scaled inputs and its finishing FMA folds 1 / xscale; finite, blocks redone, and within
    that test's 1e-5 of max |y| of float64."""
    x = rnd(1, 8, 8, 128, seed=3)
    x[0, :, 2:6, 70:90] *= 3e3
    w = rnd(32, 8, 3, 3, seed=4) / 8
    b = rnd(32, seed=11)
    U = _filters(monkeypatch, w)
    _redo_blocks()
    (got,) = _run(monkeypatch, dict(x=x, U=U, bias=b))
    redo = _redo_blocks()
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1).float()
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max()) / scale
    print(f"split5 range guard: {redo} blocks redone, max err {err:.2e} of max |y|")
    assert torch.isfinite(got).all() and redo > 0
    assert err < 1e-5, err


def test_split5_rescale_fold_is_exact(monkeypatch):
    """Inputs in {-1, 0, 1} and filters k * 9 / 64, k in {-1, 0, 1}, without bias: every intermediate of
    the split kernel is then an integer (in units of 2^-12) below 2^24: the transformed inputs
    (|V| <= 100: one f16, no lo half), the scaled transformed filters 576 k' (24 G x 24 G is
    integral; their hi + lo halves are exact), the products, the fp32 sums and both output transforms.
    So the kernel's result is the exact convolution whether the accumulators are rescaled before the
    output transform or the finished sums after it, and must equal the float64 result bit for bit."""
    g = torch.Generator(device="cpu").manual_seed(12)
    x = torch.randint(-1, 2, (1, 8, 8, 128), generator=g).float().to(dev)
    w = (torch.randint(-1, 2, (32, 8, 3, 3), generator=g).float() * (9.0 / 64.0)).to(dev)
    # the bound that makes it so: every partial sum of the main loop is below the sum over channels of
    # |V| |U 2^12| of its point, and every intermediate of the output transforms is a sub-sum of
    # |A^T| (those sums) |A|
    AT = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, 1, 2, 2, 0], [0, 1, 1, 4, 4, 0], [0, 1, 1, 8, 8, 1]], dtype=torch.float64)
    G24 = torch.tensor([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], dtype=torch.float64)
    BT = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
                       [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=torch.float64)
    U = torch.einsum("ak,oikl,bl->abio", G24, w.double().cpu() * (4096.0 / 576.0), G24)
    xp = F.pad(x.double().cpu()[0], (1, 1, 1, 1))
    d = xp.unfold(1, 6, 4).unfold(2, 6, 4)                      # [c, th, tw, 6, 6]
    V = torch.einsum("ak,ctskl,bl->abcts", BT, d, BT)
    assert float(V.abs().max()) <= 2048 and float((U - U.round()).abs().max()) == 0
    m_abs = torch.einsum("abcts,abco->abots", V.abs(), U.abs())
    y_abs = torch.einsum("ia,abots,jb->otisj", AT, m_abs, AT)
    assert float(y_abs.max()) < 2 ** 24, float(y_abs.max())
    (got,) = _run(monkeypatch, dict(x=x, U=_filters(monkeypatch, w)))
    ref64 = F.conv2d(x.double(), w.double(), padding=1)
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64)
    assert torch.equal(got, ref), float((got - ref).abs().max())

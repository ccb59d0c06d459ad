"""The mixed-precision F(4x4,3x3) kernel (conv2d_wino4.hip W4Half, block_shape 7, ops.mixed_precision).

Reference value: the numpy restatement tests/mixed_ref.py (V rounded once to f16, exact filter pairs,
fp32 sums).  Kernel and restatement differ only where the fp32 transform's last bits flip an f16
rounding (a fraction ~2^-12 of the values, ~2 % of the mode's own RMS error) and by fp32 summation
order (~1e-6 of scale), so with E = RMS(restatement - fp64 direct conv):
    RMS(gpu - restatement) <= 0.25 E   and   0.75 E <= RMS(gpu - fp64) <= 1.25 E
(the second also catches a build that rounds the filters too: 1.42 E on the CPU).

The epilogue / prologue instances (affine input, gates 1-3, pitched planes) are checked at the shapes
and tolerances of the split cases in test_gpu_wino.py, their expected values built from the plain
mixed conv's output (pinned above) plus torch's epilogue math."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mixed_ref import rms, wino4_mixed
from stereoanywhere_amd import ops
from test_split_numerics_cpu import direct

pytestmark = pytest.mark.gpu
dev = "cuda"


def rnd(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev)


def _mixed(monkeypatch, *probs, mixed=True):
    """conv2d_k3_multi on the F(4x4) kernel whatever the size, in (or out of) the mode; returns the
    results and the launches per block shape."""
    monkeypatch.setattr(ops, "_WINO4", True)
    monkeypatch.setattr(ops, "_WINO4_MIN_BLOCKS", 0)
    ops.W4_SHAPE_LAUNCHES.clear()
    with ops.mixed_precision(mixed):
        res = ops.conv2d_k3_multi(*probs)
    return res, dict(ops.W4_SHAPE_LAUNCHES)


def _redo_blocks():
    from stereoanywhere_amd import _native as N
    n = int(N.lib().sa_split_redo_blocks(1))
    assert n >= 0
    return n


_REF = {}


def _refs(N, Cin, Cout, H, W):
    """(x, w, b, restatement, fp64) of one shape, computed once (without bias)."""
    key = (N, Cin, Cout, H, W)
    if key not in _REF:
        x = rnd(N, Cin, H, W, seed=Cin + 1)
        w = rnd(Cout, Cin, 3, 3, seed=Cout + 1) / (3 * Cin ** 0.5)
        b = rnd(Cout, seed=8)
        xn, wn = x.cpu().numpy(), w.cpu().numpy()
        rest = np.stack([wino4_mixed(xn[n], wn) for n in range(N)])
        f64 = np.stack([direct(xn[n], wn) for n in range(N)])
        _REF[key] = (x, w, b, rest, f64)
    return _REF[key]


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("N,Cin,Cout,H,W", [(1, 8, 32, 8, 32),      # one chunk
                                            (2, 16, 64, 9, 36),     # two chunks (both LDS buffers), two channel
                                                                    # blocks, ragged H
                                            (1, 64, 96, 17, 52),    # eight chunks, three channel blocks
                                            (1, 16, 32, 8, 128)])   # the 8 x 128 block shape
def test_mixed_matches_restatement(monkeypatch, N, Cin, Cout, H, W, epilogue):
    x, w, b, rest, f64 = _refs(N, Cin, Cout, H, W)
    U = ops.wino_weights(w)
    assert U.u4s is not None
    (got,), shapes = _mixed(monkeypatch, dict(x=x, U=U, bias=b if epilogue else None, relu=epilogue))
    assert shapes.get(7, 0) > 0 and shapes.get(6, 0) == 0, shapes
    (_,), shapes_off = _mixed(monkeypatch, dict(x=x, U=U), mixed=False)
    assert shapes_off.get(6, 0) > 0 and shapes_off.get(7, 0) == 0, shapes_off
    if epilogue:   # bias + ReLU on both references (fp32 adds of the same bias; exact in fp64)
        bn = b.cpu().numpy()[None, :, None, None]
        rest = np.maximum(rest + bn.astype(np.float32), 0.0)
        f64 = np.maximum(f64 + bn.astype(np.float64), 0.0)
    g = got.cpu().numpy()
    assert g.dtype == np.float32 and np.isfinite(g).all()
    E = rms(rest - f64)
    d_rest, d_f64 = rms(g - rest), rms(g - f64)
    print(f"mixed {N}x{Cin}->{Cout} {H}x{W} epilogue={epilogue}: E {E:.3e}, gpu-restatement {d_rest:.3e} "
          f"({d_rest / E:.3f} E), gpu-fp64 {d_f64:.3e} ({d_f64 / E:.3f} E)")
    assert E > 0
    assert d_rest <= 0.25 * E, (d_rest, E)
    assert 0.75 * E <= d_f64 <= 1.25 * E, (d_f64, E)


def test_mixed_input_transform(monkeypatch):
    """The affine-input instance (the producer's norm + ReLU on load), test_wino4_input_transform's
    shapes and tolerances.  Expected: the plain mixed conv of the transformed input, the transform
    restated as the kernel applies it (scale s, shift t - m s, one fused multiply-add each; float64
    products rounded once give the same bits), so both convs round the same values to f16."""
    from stereoanywhere_amd import encoders
    g = torch.Generator(device="cpu").manual_seed(51)

    def r(*s):
        return torch.randn(*s, generator=g).cuda()
    xa = r(2, 96, 37, 132) * 2 + 0.7           # channel slice [16, 80) of it
    xb, xc = r(3, 32, 20, 52) + 0.3, r(1, 64, 9, 36)
    wa, wb, wc = r(64, 64, 3, 3) / 24, r(96, 32, 3, 3) / 17, r(32, 64, 3, 3) / 24
    mean, rstd = ops.plane_stats(xa[:, 16:80])
    bn = torch.nn.BatchNorm2d(32).cuda().eval()
    with torch.no_grad():
        bn.running_mean.copy_(r(32))
        bn.running_var.copy_(r(32).abs() + 0.5)
        bn.weight.copy_(r(32))
        bn.bias.copy_(r(32))
    aff_a = ops.Affine(mean, rstd, None, per_plane=True)
    aff_b = encoders.bn_affine(bn, None)
    Ua, Ub, Uc = ops.wino_weights(wa), ops.wino_weights(wb), ops.wino_weights(wc)

    def transformed(x, aff, relu):
        B, C = x.shape[:2]
        shp = (B, C, 1, 1) if aff.per_plane else (1, C, 1, 1)
        z = torch.zeros(shp, device=dev, dtype=torch.float64)
        m = z if aff.m is None else aff.m.double().view(shp)
        s = z + 1 if aff.s is None else aff.s.double().view(shp)
        t = z if aff.t is None else aff.t.double().view(shp)
        shift = (t - m * s).float().double()
        v = (x.double() * s + shift).float()
        return torch.relu(v) if relu else v

    ((ya, (ma, ra)), yb, yc), shapes = _mixed(
        monkeypatch, dict(x=xa[:, 16:80], U=Ua, in_aff=aff_a, in_act="relu", stats=True),
        dict(x=xb, U=Ub, in_aff=aff_b, in_act="relu"), dict(x=xc, U=Uc))
    assert shapes == {7: 1}, shapes
    (ea, eb, ec), shapes = _mixed(monkeypatch, dict(x=transformed(xa[:, 16:80], aff_a, True).contiguous(), U=Ua),
                                  dict(x=transformed(xb, aff_b, True), U=Ub), dict(x=xc, U=Uc))
    assert shapes == {7: 1}, shapes
    for name, y, e in (("a", ya, ea), ("b", yb, eb), ("c", yc, ec)):
        print(f"input transform {name}: max |y - expected| {float((y - e).abs().max()):.2e}")
    torch.testing.assert_close(ya, ea, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(ma, ea.mean(dim=(2, 3)).flatten(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(ra, torch.rsqrt(ea.var(dim=(2, 3), unbiased=False) + 1e-5).flatten(),
                               atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(yb, eb, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(yc, ec, atol=1e-4, rtol=1e-4)
    # it is the mode's arithmetic, not the split kernel's: off by the mode's own error from fp32
    ref_a = F.conv2d(torch.relu(F.instance_norm(xa[:, 16:80])), wa, padding=1)
    rel = float((ya - ref_a).abs().mean() / ref_a.abs().mean())
    print(f"input transform a: mean |y - fp32| / mean |y| = {rel:.2e}")
    assert 2e-4 < rel < 5e-3, rel
    # affine without activation: negative inputs pass through
    s, t = r(64).abs() + 0.5, r(64)
    aff_d = ops.Affine(None, s, t)
    (yd,), _ = _mixed(monkeypatch, dict(x=xc, U=Uc, in_aff=aff_d))
    (ed,), _ = _mixed(monkeypatch, dict(x=transformed(xc, aff_d, False), U=Uc))
    torch.testing.assert_close(yd, ed, atol=1e-4, rtol=1e-4)


def test_mixed_gru_gate_epilogues(monkeypatch):
    """Gate modes 1 and 2 (test_wino4_gru_gate_epilogues' shapes and tolerances): the expected gates
    from the plain mixed conv's output and torch's sigmoid / tanh."""
    g = torch.Generator(device="cpu").manual_seed(42)

    def r(*s):
        return torch.randn(*s, generator=g).cuda()
    for B, hd, xd, H, W in ((2, 128, 256, 40, 240), (1, 128, 128, 34, 60)):
        hxr = r(B, 2 * hd + xd, H, W)
        h, x, rh_out = hxr[:, :hd], hxr[:, hd:hd + xd], hxr[:, hd + xd:]
        ctx = r(B, 3 * hd, H, W)
        wz, wr, wq = (r(hd, hd + xd, 3, 3) / (3 * (hd + xd) ** 0.5) for _ in range(3))
        bz, br, bq = r(hd), r(hd), r(hd)
        Uzr, Uqx = ops.wino_weights(torch.cat([wz, wr]).contiguous()), ops.wino_weights(wq[:, hd:].contiguous())
        Uqh = ops.wino_weights(wq[:, :hd].contiguous())
        hx = hxr[:, :hd + xd]
        (zr_plain, qx_plain), shapes = _mixed(monkeypatch, dict(x=hx, U=Uzr, bias=torch.cat([bz, br])),
                                              dict(x=x, U=Uqx))
        assert shapes == {7: 1}, shapes
        z = torch.empty(B, hd, H, W, device=dev)
        qx = torch.empty(B, hd, H, W, device=dev)
        (zo, qxo), shapes = _mixed(monkeypatch, dict(x=hx, U=Uzr, bias=torch.cat([bz, br]), out=z,
                                                     gate=dict(mode=1, ctx=ctx, h=h, out2=rh_out)),
                                   dict(x=x, U=Uqx, out=qx))
        assert shapes == {7: 1} and zo is z and qxo is qx, shapes
        z_ref = torch.sigmoid(zr_plain[:, :hd] + ctx[:, :hd])
        r_ref = torch.sigmoid(zr_plain[:, hd:] + ctx[:, hd:2 * hd])
        torch.testing.assert_close(z, z_ref, atol=3e-5, rtol=1e-4)
        torch.testing.assert_close(rh_out, r_ref * h, atol=3e-5, rtol=1e-4)
        torch.testing.assert_close(qx, qx_plain, atol=1e-4, rtol=1e-4)
        # and it is the mode's conv underneath: z differs from the split kernel's beyond its tolerance
        z_split = torch.empty_like(z)
        _mixed(monkeypatch, dict(x=hx, U=Uzr, bias=torch.cat([bz, br]), out=z_split,
                                 gate=dict(mode=1, ctx=ctx, h=h, out2=torch.empty_like(z))), mixed=False)
        assert float((z - z_split).abs().max()) > 3e-5
        # mode 2: h <- (1 - z) h + z tanh((add + conv) + ctx), in place on h
        h0 = h.clone()
        (q_plain,), _ = _mixed(monkeypatch, dict(x=rh_out, U=Uqh, bias=bq))
        h_ref = (1 - z) * h0 + z * torch.tanh((qx + q_plain) + ctx[:, 2 * hd:])
        (ho,), shapes = _mixed(monkeypatch, dict(x=rh_out, U=Uqh, bias=bq, out=h,
                                                 gate=dict(mode=2, ctx=ctx[:, 2 * hd:], h=h, z=z, add=qx)))
        assert ho is h and shapes == {7: 1}, shapes
        torch.testing.assert_close(h, h_ref, atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("B,H,W", [(2, 136, 240), (1, 40, 64), (3, 52, 100), (1, 24, 136)])
def test_mixed_flow_head(monkeypatch, B, H, W):
    """Gate mode 3 (ops.flow_head_update) in the mode, test_flow_head_fused_matches_separate's shapes
    and tolerances: equal to the plain mixed conv1 -> conv2d_k3_narrow -> flow_update, and to torch's
    conv2 (float64) of the plain mixed conv1's output."""
    monkeypatch.setattr(ops, "_WINO4", True)
    monkeypatch.setattr(ops, "_WINO4_MIN_BLOCKS", 0)
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + H + W)

    def r(*s):
        return torch.randn(*s, generator=g).to(dev)
    h = torch.tanh(r(B, 128, H, W))
    w1, b1 = r(256, 128, 3, 3) / 34, r(256) * 0.1
    w2, b2 = r(2, 256, 3, 3) / 48, r(2) * 0.1
    U1 = ops.wino_weights(w1)
    cx0 = torch.arange(W, device=dev, dtype=torch.float32).expand(B, 1, H, W).contiguous() - 3.0 * torch.rand(
        B, 1, H, W, generator=g).to(dev)
    cx_a, flow_a = cx0.clone(), torch.full((B, 2, H, W), 7.0, device=dev)
    cx_b, flow_b = cx0.clone(), torch.full((B, 2, H, W), 7.0, device=dev)
    ops.W4_SHAPE_LAUNCHES.clear()
    with ops.mixed_precision(True):
        f1 = ops.conv2d_k3(h, U1, b1, relu=True)
        delta = ops.conv2d_k3_narrow(f1, w2, b2)
        ops.flow_update(cx_a, delta[:, 0:1], flow_a, None)
        assert ops.flow_head_update(h, U1, b1, w2, b2, cx_b, flow_b)
    assert ops.W4_SHAPE_LAUNCHES == {7: 2}, ops.W4_SHAPE_LAUNCHES
    ref = F.conv2d(f1.double(), w2.double(), b2.double(), padding=1)[:, 0:1].float()
    d_b = cx_b - cx0
    print(f"mixed flow head {B}x{H}x{W}: max |delta - ref| {float((d_b - ref).abs().max()):.2e}")
    torch.testing.assert_close(d_b, ref, atol=2e-5, rtol=1e-4)
    torch.testing.assert_close(cx_b, cx_a, atol=2e-5, rtol=1e-6)
    torch.testing.assert_close(flow_b, flow_a, atol=2e-5, rtol=1e-5)
    assert float(flow_b[:, 1].abs().max()) == 0.0


def test_mixed_pitched_planes(monkeypatch):
    """Pitched planes (W 10 at pitch 12): the conv of the first W columns, the pad columns of the output
    zero.  Expected: the plain mixed conv of the same 12-column planes taken as a dense image (its zero
    columns 10-11 act as the right padding), at test_wino4_pitched_planes' tolerance."""
    g = torch.Generator(device="cpu").manual_seed(91)

    def r(*s):
        return torch.randn(*s, generator=g).cuda()
    B, Cin, Cout, H, W, P = 2, 64, 64, 9, 10, 12
    x = torch.zeros(B, Cin, H, P, device=dev)
    x[..., :W] = r(B, Cin, H, W)
    w, b = r(Cout, Cin, 3, 3) / (3 * Cin ** 0.5), r(Cout)
    U = ops.wino_weights(w)
    (ya,), shapes = _mixed(monkeypatch, dict(x=x, U=U, bias=b, relu=True, width=W))
    assert shapes == {7: 1}, shapes
    (ed,), _ = _mixed(monkeypatch, dict(x=x, U=U, bias=b, relu=True))
    assert ya.shape == (B, Cout, H, P)
    assert float(ya[..., W:].abs().max()) == 0.0
    torch.testing.assert_close(ya[..., :W], ed[..., :W], atol=1e-4, rtol=1e-4)
    ref = torch.relu(F.conv2d(x[..., :W], w, b, padding=1))
    rel = float((ya[..., :W] - ref).abs().mean() / ref.abs().mean())
    assert 2e-4 < rel < 5e-3, rel


def test_mixed_range_guard(monkeypatch):
    """Inputs whose transformed values pass the f16 range (magnitude 3000, as
    test_wino4_split_range_guard): hi overflows to inf, the staged sums turn non-finite and the block
    runs again on inputs scaled by a power of two.  Finite, blocks redone, and no further from float64
    than 1.25 x the restatement (run on the input times the guard's power of two, which changes no
    f16 rounding above the subnormal range, and scaled back)."""
    x = rnd(2, 64, 36, 256, seed=3)
    x[0, :, 4:12, 70:90] *= 3000.0
    w = rnd(96, 64, 3, 3, seed=4) / 24
    U = ops.wino_weights(w)
    assert U.u4s is not None
    _redo_blocks()
    (y,), shapes = _mixed(monkeypatch, dict(x=x, U=U))
    redo = _redo_blocks()
    assert shapes == {7: 1}, shapes
    assert torch.isfinite(y).all()
    assert redo > 0, redo
    xn, wn = x.cpu().numpy(), w.cpu().numpy()
    e2 = int(np.frexp(100.0 * np.abs(xn).max())[1])
    sc = np.float32(2.0 ** (15 - e2))
    rest = np.stack([wino4_mixed(xn[n] * sc, wn) for n in range(2)]) / sc
    f64 = np.stack([direct(xn[n], wn) for n in range(2)])
    assert np.isfinite(rest).all()
    E, d = rms(rest - f64), rms(y.cpu().numpy() - f64)
    print(f"mixed range guard: {redo} blocks redone; gpu-fp64 {d:.3e}, restatement-fp64 {E:.3e} ({d / E:.3f} E)")
    assert d <= 1.25 * E, (d, E)

"""Every 3-D kernel of the fused mono hourglass (csrc/conv3d_fused.hip, conv3d_mfma.hip,
conv3d_s2mf.hip, mono_volume.hip), one at a time, against the float64 CPU reference of
tests/hourglass_ref.py (pinned to the torch Hourglass by tests/test_hourglass_ref_cpu.py): outputs
and InstanceNorm statistics, every element, at shapes taken from the kernels' tile sizes.

Inputs: B = 2, seeded; mean ~ 0.1 N(0,1), rstd in [0.5, 1.5), gates in (0, 1), weights scaled by
sqrt(2 / (K Cin)).  Channels 1 and 2 of every normed input carry mean = -3 / +3 at rstd = 1, so
T(0) = 3 (and lrelu(-3)): a kernel that pads before the transform is wrong at the border by the
order of the data.

Tolerances are elementwise and derived (u = 2^-24, ``mag`` = the reference computation on absolute
values); the derivation is in each test's docstring and every test prints max err / bound.
Statistics are compared with float64 statistics of the kernel's own output (_check_stats).
Reference: hourglass.py:13-91, submodule.py:25-53, :113-140, stereoanywhere.py:136, :161-166."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hourglass_ref as H
from stereoanywhere_amd import _native as N, ops

pytestmark = pytest.mark.gpu
dev = "cuda"
U = H.U
SLOPE = 0.01
CELL = 10 * U * 1.73 / math.sqrt(3.0)   # |cell - oracle cell|, see test_conv3d_onehot


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _input(cin, shape, seed, norm=True, act=True, gate=False, B=2, offset=0.0):
    """-> (ops.VolAct on the GPU, its float64 T(x) on the CPU, |mean * rstd| as a volume).
    ``offset``: channel 0 is shifted by it (through its mean, or raw), for the large-offset
    statistics cases."""
    D, Hh, W = shape
    rng = np.random.default_rng(seed)
    x = f32(rng.standard_normal((B, cin, D, Hh, W)))
    mean, rstd = f32(rng.standard_normal((B, cin)) * 0.1), f32(rng.random((B, cin)) + 0.5)
    if cin > 2:   # the zero-padding probes
        mean[:, 1], rstd[:, 1], mean[:, 2], rstd[:, 2] = -3.0, 1.0, 3.0, 1.0
    if offset and norm:
        mean[:, 0], rstd[:, 0] = -offset, 1.0
    elif offset:
        x[:, 0] += offset
    nrm = (mean.reshape(-1), rstd.reshape(-1)) if norm else None
    gt = (f32(0.05 + 0.9 * rng.random((B, cin, Hh, W))), f32(0.05 + 0.9 * rng.random((B, cin, Hh, D)))) if gate else None
    v = ops.VolAct(x.to(dev), None if nrm is None else tuple(t.to(dev) for t in nrm), act,
                   None if gt is None else tuple(t.to(dev) for t in gt))
    mr = (mean.double() * rstd.double()).abs().reshape(B, cin, 1, 1, 1).expand(B, cin, D, Hh, W)
    return v, H.T(x, nrm, act, gt, SLOPE), H.T(mr, None, False, gt)


def _weights(cin, cout, seed, k=27, offset=False):
    rng = np.random.default_rng(1000 + seed)
    w = f32(rng.standard_normal((cin, k, cout) if k > 1 else (cin, cout)) * (2.0 / (k * cin)) ** 0.5)
    if offset:   # channel 0 through the centre tap alone, the same sign for every output
        w[0] = 0.0
        if k > 1:
            w[0, k // 2] = 1.0
        else:
            w[0] = 1.0
    return w


def _check(name, got, ref, bound):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max err {float(err.max()):.3g}, max err/bound {ratio:.3g}")
    assert bool((err <= bound).all()), (name, float(err.max()), ratio)
    return ratio


def _check_stats(name, v, nf, eps=1e-5):
    """The op's (mean, rstd) against float64 statistics of its own returned output.  A thread sums
    at most ``nf`` fp32 values of x and of x^2 (one rounding per term), everything above is
    float64 and the results are rounded to fp32 once:
      |mean - m64| <= (nf + 1) u E|x| + u |m64|
      var = E[x^2] - m^2 is off by at most (nf + 2) u (E[x^2] + 2 |m| E|x|), and rstd = (var + eps)^-1/2:
      |rstd / r64 - 1| <= 1/2 [(nf + 2) u (E[x^2] + 2 |m| E|x|) + u eps] / (var + eps) + u
    (u eps: the C ABI takes eps as a float, 1e-5 rounded to fp32)."""
    y = v.raw.detach().cpu().double()
    m64, r64 = H.stats(y, eps)
    ex, ex2 = y.abs().mean(dim=(2, 3, 4)).reshape(-1), (y * y).mean(dim=(2, 3, 4)).reshape(-1)
    bm = (nf + 1) * U * ex + U * m64.abs()
    br = 0.5 * ((nf + 2) * U * (ex2 + 2 * m64.abs() * ex) + U * eps) * r64 ** 2 + U
    em = (v.norm[0].cpu().double() - m64).abs()
    er = (v.norm[1].cpu().double() / r64 - 1).abs()
    print(f"{name} stats: mean err/bound {float((em / bm.clamp_min(1e-300)).max()):.3g}, "
          f"rstd err/bound {float((er / br).max()):.3g}, max |mean| rstd {float((m64.abs() * r64).max()):.3g}")
    assert bool((em <= bm).all()) and bool((er <= br).all()), (name, float(em.max()), float(er.max()))
    return float((m64.abs() * r64).max())


def _distinct(shapes):
    """The table's shapes, plus a variant with H + 1 where two of a shape's sizes coincide."""
    out = []
    for s in shapes:
        out.append(s)
        if len(set(s)) < 3 and s[0] > 2:
            out.append((s[0], s[1] + 1, s[2]))
    return out


def _td(cout):   # conv_geo's planes per thread at stride 1
    return 8 if cout <= 8 else (2 if cout >= 32 else 4)


def _direct_cases():
    for cin, cout in ((8, 8), (8, 2), (16, 16), (32, 32)):
        td = _td(cout)
        for shape in _distinct([(1, 1, 1), (td + 1, 5, 63), (2 * td + 1, 3, 125)]):
            for gated in (False, True):
                yield cin, cout, 1, shape, "gated" if gated else "act"
    for cin, cout in ((8, 16), (16, 32)):
        for shape in ((1, 1, 1), (4, 17, 62), (5, 18, 63), (3, 9, 125)):
            for mode in (("raw",) if cin == 8 else ()) + ("act", "gated"):
                yield cin, cout, 2, shape, mode


@pytest.mark.parametrize("cin,cout,stride,shape,mode", list(_direct_cases()))
def test_conv3d_direct(cin, cout, stride, shape, mode):
    """sa_conv3d, every instance, stride 1 (62 x 4 x td tiles) and 2 (31 x 8 x 2): one tile, one
    tile plus one element, two tiles and a ragged third, and the one-voxel volume.
    fp32 direct sum of K = 27 Cin terms: |got - ref| <= (K + 6) u mag (K accumulations; the 6 covers
    the roundings of T - subtract, scale, slope, gl * gr, the gate product - and the comparison's)."""
    seed = cin + 3 * cout + sum(shape)
    v, tx, _ = _input(cin, shape, seed, norm=mode != "raw", act=mode != "raw", gate=mode == "gated")
    w = _weights(cin, cout, seed)
    ref, mag = H.conv3(tx, w, stride)
    a = ops.conv3d(v, w.to(dev), cout, stride=stride, slope=SLOPE)
    name = f"conv3d {cin}->{cout} s{stride} {shape} {mode}"
    _check(name, a.raw, ref, (27 * cin + 6) * U * mag)
    _check_stats(name, a, _td(cout) if stride == 1 else 2)


# B^T and A^T of F(4,3) at the points 0, +-1, +-2, inf as bt6 / at6 of conv3d_fused.hip state them
_BT = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0],
                    [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=torch.float64)
_AT = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]],
                   dtype=torch.float64)


def _f43(tx, w_wd, absolute):
    """y = A^T [sum over (ci, kh, kw) of (G g) . (B^T d)] along D in 4-plane groups, in float64, with
    the kernel's transformed weights w_wd [Cin][3][3][6][Cout]; ``absolute``: every factor by its
    absolute value (the running-error magnitude M)."""
    B, C, D, Hh, W = tx.shape
    nt = (D + 3) // 4
    Bt, At, Ug = (_BT.abs(), _AT.abs(), w_wd.double().abs()) if absolute else (_BT, _AT, w_wd.double())
    x = F.pad(tx.abs() if absolute else tx, (1, 1, 1, 1, 1, 4 * nt + 1 - D))
    V = torch.einsum("pq,bcthwq->bcpthw", Bt, x.unfold(2, 6, 4))
    M = 0
    for kh in range(3):
        for kw in range(3):
            M = M + torch.einsum("cpo,bcpthw->bopthw", Ug[:, kh, kw], V[..., kh:kh + Hh, kw:kw + W])
    return torch.einsum("ip,bopthw->botihw", At, M).reshape(B, -1, 4 * nt, Hh, W)[:, :, :D]


WD_SHAPES = [(1, 1, 1), (1, 5, 63), (3, 5, 63), (4, 3, 125), (5, 3, 63), (9, 5, 63), (17, 3, 125)]
WD_INST = [(8, 8, False), (8, 8, True), (8, 2, False), (8, 2, True), (16, 16, False), (16, 16, True),
           (32, 32, False)]


@pytest.mark.parametrize("shape", WD_SHAPES)
@pytest.mark.parametrize("cin,cout,gated", WD_INST)
def test_conv3d_wd(cin, cout, gated, shape):
    """sa_conv3d_wd (F(4,3) along D in 4-plane groups, 62 x 4 tiles), variants 0-3, D in
    {1, 3, 4, 5, 9, 17}.  Running-error bound of y = A^T[(G g) . (B^T d)]:
    M = |A^T| sum_{ci,kh,kw} (|G g| . |B^T| |T(d)|) in float64 with the kernel's own matrices, and
    |got - ref| <= (9 Cin + 17) u M: 9 Cin accumulations per transform point; along one output's chain
    at most 5 + 3 + 1 + 4 roundings of T, B^T, G g and A^T, the rest for the second-order terms."""
    seed = cin + cout + sum(shape) + gated
    v, tx, _ = _input(cin, shape, seed, gate=gated)
    w = _weights(cin, cout, seed)
    w_wd = ops.conv3d_wd_weights(w)
    ref, _ = H.conv3(tx, w)
    # the matrices restated above do compute the convolution
    assert float((_f43(tx, w_wd, False) - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
    bound = (9 * cin + 17) * U * _f43(tx, w_wd, True)
    for variant in range(4):
        N.lib().sa_conv3d_wd_set_variant(variant)
        try:
            a = ops.conv3d_wd(v, w_wd.to(dev), cout, slope=SLOPE)
        finally:
            N.lib().sa_conv3d_wd_set_variant(0)
        name = f"conv3d_wd v{variant} {cin}->{cout} {shape} {'gated' if gated else 'act'}"
        _check(name, a.raw, ref, bound)
        _check_stats(name, a, 8 if cin == 8 else 4)


def _split_bound(tx, mr, w, stride, ref_mag):
    """Split-f16 MFMA (header of conv3d_mfma.hip): activation and 2^12-scaled weight as f16 hi + lo
    (11 bits each), hi*hi + hi*lo + lo*hi exact products accumulated in fp32, lo*lo dropped:
      [(K + 6) u + 3 2^-22] mag          K accumulations; each operand's split and the dropped product
      + 2^-25 sum |w|                    the lo part of an activation below the f16 normal range
      + 2^-37 sum |T(x)|                 the same for the lo part of a weight, at its 2^12 scale
      + u sum |w| |mean rstd| (gated)    the kernels form T as fma(x, rstd, -mean * rstd): the product
                                         mean * rstd is rounded once, an error relative to it, not to T
    (sums over the taps inside the volume).  The last two terms are not in the fp32 kernels' bound:
    they follow from the weight split and from the fma form of the transform in the kernels."""
    K = 27 * tx.shape[1]
    one = torch.ones_like(tx)
    return ((K + 6) * U + 3 * 2.0 ** -22) * ref_mag + 2.0 ** -25 * H.conv3(one, w, stride)[1] \
        + 2.0 ** -37 * H.conv3(tx, torch.ones_like(w), stride)[1] + U * H.conv3(mr, w, stride)[1]


def _mf_cases():
    for cin, th, tw in ((8, 8, 64), (16, 4, 64), (32, 4, 32)):
        for shape in ((1, 1, 1), (3, th + 1, tw + 1), (11, 2 * th + 1, 2 * tw + 3)):
            for planes in (0, 3, 4):
                yield cin, shape, planes


@pytest.mark.parametrize("cin,shape,planes", list(_mf_cases()))
def test_conv3d_mf(cin, shape, planes):
    """sa_conv3d_mf (TH x TW tiles of 8 x 64, 4 x 64, 4 x 32; D ranges of ``planes`` planes through
    sa_conv3d_mf_set_planes, 0 = automatic) within _split_bound; a thread sums 16 (8 -> 8) or 8 fp32
    values into its float64 statistics."""
    seed = cin + sum(shape) + planes
    v, tx, mr = _input(cin, shape, seed)
    w = _weights(cin, cin, seed)
    ref, mag = H.conv3(tx, w)
    table = ops.conv3d_mf_weights(w.to(dev))
    assert table is not None
    N.lib().sa_conv3d_mf_set_planes(planes)
    try:
        a = ops.conv3d_mf(v, table, cin, slope=SLOPE)
    finally:
        N.lib().sa_conv3d_mf_set_planes(0)
    name = f"conv3d_mf {cin}->{cin} {shape} planes {planes}"
    _check(name, a.raw, ref, _split_bound(tx, mr, w, 1, mag))
    _check_stats(name, a, 16 if cin == 8 else 8)


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 3, 5), (9, 17, 66), (6, 10, 33)])
def test_conv3d_s2mf(shape, gated):
    """sa_conv3d_s2mf (stride 2, 16 -> 32, 4 x 16 output tiles: Ho not a multiple of 4, Wo not of 16
    or 4) within _split_bound; a thread sums 8 fp32 values into its statistics."""
    seed = sum(shape) + gated
    v, tx, mr = _input(16, shape, seed, gate=gated)
    w = _weights(16, 32, seed)
    ref, mag = H.conv3(tx, w, 2)
    table = ops.conv3d_s2mf_weights(w.to(dev))
    assert table is not None
    a = ops.conv3d_s2(v, w.to(dev), table, 32, slope=SLOPE)
    name = f"conv3d_s2mf {shape} {'gated' if gated else 'act'}"
    _check(name, a.raw, ref, _split_bound(tx, mr, w, 2, mag))
    _check_stats(name, a, 8)


def _records(B, Hh, W1, W2, seed, one_bin=False):
    """Depth maps as _onehot_case of test_gpu_ops.py (three bins, exact bin edges, mde == 1.0 in no
    bin) and their normals from the oracle; ``one_bin``: every pixel in bin 2."""
    rng = np.random.default_rng(seed)
    if one_bin:
        m2 = (0.26 + 0.1 * rng.random((B, 1, Hh, W1))).astype(np.float32)
        m3 = (0.26 + 0.1 * rng.random((B, 1, Hh, W2))).astype(np.float32)
    else:
        m2 = (np.floor(rng.random((B, 1, Hh, W1)) * 3) / 8 + 0.03).astype(np.float32)
        m3 = (np.floor(rng.random((B, 1, Hh, W2)) * 3) / 8).astype(np.float32)
        m2[0, 0, 0, :4] = [1.0, 0.0, 0.5, 0.375][:min(4, W1)]
        m3[0, 0, min(1, Hh - 1), :4] =[1.0, 0.125, 0.5, 0.999][:min(4, W2)]
    return H.normals(m2, 2.0), H.normals(m3, 2.0), m2, m3


def _onehot(rec):
    return ops.OneHotVolume(*(f32(a).to(dev) for a in rec), 8, 1.73)


@pytest.mark.parametrize("shape", [(6, 9, 130), (5, 3, 7)])
def test_conv3d_onehot(shape):
    """sa_conv3d_onehot (8 bins -> 16, stride 2, 64 x 4 x 2 output tiles) against the stride-2 conv
    of the oracle's masked volume.  One non-zero bin per tap, so K = 27: (K + 6) u mag; and the cell
    itself, 1.73 (nL . nR) / sqrt(3) of unit normals in fp32, is rounded by the kernel and by the
    oracle each within 3 u (the dot product, relative to |nL||nR| = 1) + 2 u (division, gain):
    + 10 u 1.73 / sqrt(3) sum |w| over the matching taps."""
    D, Hh, W = shape
    rec = _records(2, Hh, W, D, 5 + W)
    dense, hit = H.masked_volume(*rec)
    assert tuple(dense.shape) == (2, 8, D, Hh, W) and int((dense != 0).sum()) > dense.numel() // 40
    w = _weights(8, 16, W)
    ref, mag = H.conv3(dense.double(), w, 2)
    a = ops.conv3d(_onehot(rec), w.to(dev), 16, stride=2, slope=SLOPE)
    _check(f"conv3d_onehot {shape}", a.raw, ref, (27 + 6) * U * mag + CELL * H.conv3(hit.double(), w, 2)[1])
    _check_stats(f"conv3d_onehot {shape}", a, 2)


MODES = [(n, a, gt) for n in (False, True) for a in (False, True) for gt in (False, True)]


@pytest.mark.parametrize("norm,act,gate", MODES)
@pytest.mark.parametrize("shape", [(3, 5, 7), (4, 6, 65)])
@pytest.mark.parametrize("cin,cout", [(16, 8), (32, 16)])
def test_conv3d_pointwise(cin, cout, shape, norm, act, gate):
    """sa_conv3d_pointwise with every combination of norm, act and gate: an fp32 sum of K = Cin
    terms, |got - ref| <= (K + 6) u mag."""
    seed = cin + sum(shape) + 4 * norm + 2 * act + gate
    v, tx, _ = _input(cin, shape, seed, norm, act, gate)
    w = _weights(cin, cout, seed, k=1)
    ref, mag = H.pointwise(tx, w)
    got = ops.conv3d_pointwise(v, w.to(dev), cout, slope=SLOPE)
    _check(f"pointwise {cin}->{cout} {shape} norm {norm} act {act} gate {gate}", got, ref, (cin + 6) * U * mag)


def _upcat_bound(ca, cu, m):
    """out = Wa.T(a) + up(p), p = Wu.T(u) stored in fp32 at the low resolution:
      (Ca + 6) u mag_a                the direct sum Wa.T(a)
      (Cu + 6) u up(|Wu|.|T(u)|)      p's own error (the interpolation weights are convex)
      7 u up(|p|)                     the lerp chain: 2 roundings per axis and the final add
      3 u sum_axis n range_axis       the source coordinate s * dst in fp32: s = (n - 1) / (N - 1) and the
                                      product are rounded once each, 1 - frac once more, so an axis
                                      weight is off by at most 3 u n (n = the low-resolution size along
                                      it), which moves the value by at most that times the step of p
                                      between neighbouring low-resolution cells along the axis."""
    coord = sum(n * r for n, r in zip(m["n"], m["range"]))
    return ((ca + 6) * m["a"] + (cu + 6) * m["pm"] + 7 * m["p"] + 3 * coord) * U


UPCAT_SHAPES = [((8, 12, 64), (4, 6, 32)), ((9, 6, 130), (5, 3, 65)), ((10, 7, 67), (3, 2, 20)), ((2, 2, 2), (1, 1, 1))]


@pytest.mark.parametrize("shape,low", UPCAT_SHAPES)
@pytest.mark.parametrize("form", ["8x8 raw", "16x16 gated", "onehot"])
def test_conv3d_pointwise_upcat(form, shape, low):
    """sa_conv3d_pointwise_upcat <8, 8, false> (a raw), <16, 16, true> (a and u normed, activated and
    gated) and the one-hot form (64 x 4 x 4 tiles, low-resolution footprint 4 x 4 x 34): full tiles
    at scale ~1/2, odd sizes, a factor above 2 and the smallest volume, within _upcat_bound (the
    one-hot form with K = 1 and the cell term of test_conv3d_onehot); a thread sums 4 fp32 values."""
    D, Hh, W = shape
    seed = sum(shape) + len(form)
    ca, cu, cout = (16, 32, 16) if form == "16x16 gated" else (8, 16, 8)
    u, tu, _ = _input(cu, low, seed + 1, gate=True)
    wa, wu = _weights(ca, cout, seed, k=1), _weights(cu, cout, seed + 1, k=1)
    extra = 0.0
    if form == "onehot":
        rec = _records(2, Hh, W, D, seed)
        dense, hit = H.masked_volume(*rec)
        a, ta = _onehot(rec), dense.double()
        extra = CELL * H.pointwise(hit.double(), wa)[1]
    else:
        a, ta, _ = _input(ca, shape, seed, norm=ca == 16, act=ca == 16, gate=ca == 16)
    ref, m = H.upcat(ta, tu, wa, wu)
    r = ops.conv3d_pointwise_upcat(a, u, wa.to(dev), wu.to(dev), cout, slope=SLOPE)
    name = f"upcat {form} {shape} <- {low}"
    _check(name, r.raw, ref, _upcat_bound(1 if form == "onehot" else ca, cu, m) + extra)
    _check_stats(name, r, 4)


@pytest.mark.parametrize("norm,act,gate", MODES)
def test_vol_apply(norm, act, gate):
    """sa_vol_apply = T alone: at most 5 roundings, |got - ref| <= 6 u |T(x)|."""
    v, tx, _ = _input(4, (3, 5, 7), 4 * norm + 2 * act + gate, norm, act, gate)
    got = ops.vol_apply(v, slope=SLOPE)
    assert got.norm is None and not got.act and got.gate is None
    _check(f"vol_apply norm {norm} act {act} gate {gate}", got.raw, tx, 6 * U * tx.abs())


@pytest.mark.parametrize("parts", [1, 255, 256, 257, 1000])
def test_instnorm_finalize(parts):
    """sa_instnorm_finalize (a 256-thread strided sum, then a tree) on synthetic float64 partials
    against sum / count in float64 (math.fsum): the float64 sums carry at most (parts + 3) 2^-53
    relative error each, so var is off by that times E[x^2] + 2 m^2, eps reaches the kernel as a
    float (off by u eps), and both results are rounded to fp32 once.  Channel 1 has |mean| = 30 std;
    channel 2 has var < eps."""
    rng = np.random.default_rng(parts)
    bc, per, eps = 3, 7, 1e-5
    y = rng.standard_normal((bc, parts, per)) * np.array([1.0, 1.0, 1e-3])[:, None, None] \
        + np.array([0.1, 30.0, 0.0])[:, None, None]
    part = np.stack([y.sum(-1), (y * y).sum(-1)], -1)   # [bc][parts][2]
    count = parts * per
    mean, rstd = ops.instnorm_finalize(torch.from_numpy(part.reshape(-1)).to(dev), bc, parts, count, eps)
    for c in range(bc):
        m = math.fsum(part[c, :, 0]) / count
        e2 = math.fsum(part[c, :, 1]) / count
        var = e2 - m * m
        d = (parts + 3) * 2.0 ** -53
        em, bm = abs(float(mean[c]) - m), (U + d) * abs(m)
        er = abs(float(rstd[c]) * math.sqrt(var + eps) - 1)
        br = 0.5 * (d * (e2 + 2 * m * m) + U * eps) / (var + eps) + U + 2.0 ** -52
        print(f"finalize parts {parts} ch {c}: mean err/bound {em / bm:.3g}, rstd err/bound {er / br:.3g}")
        assert em <= bm and er <= br, (c, em, bm, er, br)


@pytest.mark.parametrize("W1,shift", [(20, None), (21, None), (23, None), (20, "n2"), (20, "m2")])
def test_mono_masked_volume(W1, shift):
    """sa_mono_masked_volume on its 4-wide path (W1 % 4 == 0, 16-byte aligned pointers) and its
    scalar path (W1 = 21, 23; a 4-byte-offset view of the normals or of the depth at W1 = 20)
    against the oracle's volume, as test_normals_masks_and_masked_volume compares it."""
    B, Hh, W2 = 2, 6, 18
    n2, n3, m2, m3 = _records(B, Hh, W1, W2, W1)
    t = {k: f32(a).to(dev) for k, a in (("n2", n2), ("n3", n3), ("m2", m2), ("m3", m3))}
    if shift:
        buf = torch.empty(t[shift].numel() + 1, device=dev, dtype=torch.float32)
        buf[1:] = t[shift].reshape(-1)
        t[shift] = buf[1:].view(t[shift].shape)
        assert t[shift].data_ptr() % 16 == 4 and t[shift].is_contiguous()
    out = ops.mono_masked_volume(t["n2"], t["n3"], t["m2"], t["m3"], 8, 1.73).cpu().numpy()
    ref, hit = H.masked_volume(n2, n3, m2, m3)
    assert out.shape == tuple(ref.shape) == (B, 8, W2, Hh, W1) and int((ref != 0).sum()) > ref.numel() // 40
    print(f"masked volume W1 {W1} shift {shift}: max err {float(np.abs(out - ref.numpy()).max()):.3g}")
    np.testing.assert_allclose(out, ref.numpy(), atol=1e-6, rtol=0)
    assert np.all(out[hit.numpy() == 0] == 0)   # outside the matching bins the volume is exactly zero


LARGE = ["conv3d s1", "conv3d s2", "conv3d_wd", "conv3d_mf", "conv3d_s2mf", "conv3d_onehot", "upcat", "upcat onehot"]


@pytest.mark.parametrize("kernel", LARGE)
def test_stats_large_offset(kernel):
    """One case per statistics-producing kernel whose output has |mean| >= 15 std (about 30: input
    channel 0 sits at an offset of 50 and reaches every output through one positive centre weight;
    the one-hot volume has every pixel in one bin, cells ~ 1), where E[x^2] - m^2 cancels: outputs
    within the kernel's bound, statistics within _check_stats'."""
    shape, off = (9, 6, 70), 50.0
    D, Hh, W = shape
    if kernel in ("conv3d s1", "conv3d s2", "conv3d_wd", "conv3d_mf", "conv3d_s2mf"):
        cin, cout, stride, nf = {"conv3d s1": (8, 8, 1, 8), "conv3d s2": (8, 16, 2, 2), "conv3d_wd": (16, 16, 1, 4),
                                 "conv3d_mf": (8, 8, 1, 16), "conv3d_s2mf": (16, 32, 2, 8)}[kernel]
        v, tx, mr = _input(cin, shape, 77, offset=off)
        w = _weights(cin, cout, 77, offset=True)
        ref, mag = H.conv3(tx, w, stride)
        if kernel == "conv3d_wd":
            w_wd = ops.conv3d_wd_weights(w)
            a, bound = ops.conv3d_wd(v, w_wd.to(dev), cout, slope=SLOPE), (9 * cin + 17) * U * _f43(tx, w_wd, True)
        elif kernel == "conv3d_mf":
            a, bound = ops.conv3d_mf(v, ops.conv3d_mf_weights(w.to(dev)), cout, slope=SLOPE), _split_bound(tx, mr, w, 1, mag)
        elif kernel == "conv3d_s2mf":
            a = ops.conv3d_s2(v, w.to(dev), ops.conv3d_s2mf_weights(w.to(dev)), cout, slope=SLOPE)
            bound = _split_bound(tx, mr, w, 2, mag)
        else:
            a, bound = ops.conv3d(v, w.to(dev), cout, stride=stride, slope=SLOPE), (27 * cin + 6) * U * mag
    elif kernel == "conv3d_onehot":
        rec = _records(2, Hh, W, D, 78, one_bin=True)
        dense, hit = H.masked_volume(*rec)
        w = _weights(8, 16, 78) * 0.02
        w[2, 13] = 1.0
        ref, mag = H.conv3(dense.double(), w, 2)
        a, nf = ops.conv3d(_onehot(rec), w.to(dev), 16, stride=2, slope=SLOPE), 2
        bound = (27 + 6) * U * mag + CELL * H.conv3(hit.double(), w, 2)[1]
    else:
        u, tu, _ = _input(16, (5, 3, 35), 79, gate=True)
        wa, wu, nf, extra = _weights(8, 8, 79, k=1, offset=kernel == "upcat"), _weights(16, 8, 80, k=1), 4, 0.0
        if kernel == "upcat":
            x, ta, _ = _input(8, shape, 79, norm=False, act=False, offset=off)
        else:
            rec = _records(2, Hh, W, D, 79, one_bin=True)
            dense, hit = H.masked_volume(*rec)
            x, ta, wu = _onehot(rec), dense.double(), wu * 0.02
            wa[2] = 1.0
            extra = CELL * H.pointwise(hit.double(), wa)[1]
        ref, m = H.upcat(ta, tu, wa, wu)
        a = ops.conv3d_pointwise_upcat(x, u, wa.to(dev), wu.to(dev), 8, slope=SLOPE)
        bound = _upcat_bound(1 if kernel == "upcat onehot" else 8, 16, m) + extra
    _check(f"large offset {kernel}", a.raw, ref, bound)
    assert _check_stats(f"large offset {kernel}", a, nf) >= 15.0

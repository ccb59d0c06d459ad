"""The HIP ops across the 2^31-element and 2 GiB offset lines.

(a) Far batch strides (tests/large_offsets_util.py): every row of FAR_ROWS calls its entry point with B = 2 on
    views of two 8.6 GB arenas whose batch stride is 2^31 + 64 floats, with the far stride on one parameter at
    a time and then on all of them, and asks for the bits of the same call on dense tensors.
(b) Dense totals past the lines: one seeded sample replicated along the batch until the tensor named in the
    case crosses 2^31 floats (or a dispatch line in bytes).  Every replica of every output must equal replica 0
    bit for bit, compared on the GPU replica by replica, and replica 0 must equal the one-sample run.  Where
    the batch cannot be replicated (the lookup's B = 1 pyramids on both sides of the 2 GiB dispatch) or the two
    sides run different kernels (the correlation volume on both sides of its 2 GiB feature-map dispatch), the
    first row, the last row and the row that straddles the line are compared with the op's float64
    restatement at its own test's tolerance.

A case holds at most 24 GiB of device memory, frees everything before the next, and prints its peak allocation
(pytest --durations gives its wall time); it skips only when the device has less free memory than it needs,
and says how much that is.
"""
import numpy as np
import pytest
import torch

import large_offsets_util as U
from invariance_util import bits
from oracle import ops_ref as R
from stereoanywhere_amd import _native as N, ops
from test_gpu_ops import TOL_LOOKUP, TOL_SOFTARGMIN_CONF

pytestmark = pytest.mark.gpu
dev = "cuda"
LINE = 1 << 31
GIB = 1 << 30


def need(gib):
    """Skip (saying what was needed) only when the device cannot hold the case."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    assert gib <= 24, "a case holds at most 24 GiB"
    if free < gib * GIB:
        print(f"needs {gib} GiB of device memory, {free / GIB:.1f} GiB are free")
        pytest.skip(f"needs {gib} GiB of device memory, {free / GIB:.1f} GiB are free")
    torch.cuda.reset_peak_memory_stats()


def done(label):
    """(the case's wall time is pytest's own --durations figure: the parity gate reads no clock)"""
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() / GIB
    print(f"[large offsets] {label}: peak {peak:.2f} GiB")
    assert peak <= 24.0, f"{label} held {peak:.2f} GiB"
    torch.cuda.empty_cache()


def rep(x, R_):
    """The one sample x [1, ...] R_ times along the batch, contiguous on the device."""
    x = torch.as_tensor(x).to(dev)
    assert x.shape[0] == 1
    return x.expand(R_, *x.shape[1:]).contiguous()


def assert_replicas(out, one, R_, label):
    """out [R_ * n, ...] or [R_, ...]: replica 0 equals the one-sample result `one` (None: the one-sample run
    takes another kernel, and the case compares with float64 instead), every replica equals replica 0; on
    bits, on the GPU, replica by replica (nothing left out)."""
    assert out.is_contiguous() and out.numel() % R_ == 0
    o = out.view(R_, -1)
    first = bits(o[0])
    if one is not None:
        assert one.numel() == first.numel(), f"{label}: the one-sample result has another size"
        assert torch.equal(first, bits(one.reshape(-1))), f"{label}: replica 0 differs from the one-sample run"
    bad = [b for b in range(1, R_) if not torch.equal(bits(o[b]), first)]
    assert not bad, f"{label}: {len(bad)} of {R_} replicas differ from replica 0, first {bad[0]}"


# ------------------------------------------------------------------- (b) correlation volume and pyramid
def fmaps(C, H, W1, W2, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((1, C, H, W1)).astype(np.float32), rng.standard_normal((1, C, H, W2)).astype(np.float32))


def test_truncated_pyramid_past_2_31_floats():
    """sa_corr_volume_pyramid, truncated, 4 levels: 36 x 32 x 1024 rows of 1920 floats = 2.26e9 floats."""
    need(11)
    C, H, W, B = 16, 32, 1024, 36
    f2, f3 = fmaps(C, H, W, W, 1)
    rng = np.random.default_rng(2)
    d, m = (rng.random((1, 1, H, W)) * 40).astype(np.float32), rng.random((1, 1, H, W)).astype(np.float32)
    one = ops.corr_volume_pyramid(*(rep(x, 1) for x in (f2, f3)), 4, rep(d, 1), rep(m, 1), 0.9)
    out = ops.corr_volume_pyramid(rep(f2, B), rep(f3, B), 4, rep(d, B), rep(m, B), 0.9)
    assert out.shape[1] == 1920 and out.numel() > LINE
    # the rows' padding to 4 floats is never written: level cells only (1920 = 1024 + 512 + 256 + 128)
    assert ops.pyramid_geometry(W, 4)[1][-1] + ops.pyramid_geometry(W, 4)[2][-1] == 1920
    assert_replicas(out, one, B, "truncated pyramid")
    del out, one
    done("corr_volume_pyramid truncated, 2.26e9 floats")


def test_sheared_pyramid_past_2_31_floats():
    """sa_corr_volume_pyramid_sheared: 18 x 32 slices of 3.93e6 floats = 2.26e9 floats.  The cells outside a
    level are never written, so the destination starts as zeros in both runs."""
    need(11)
    C, H, W, B = 16, 32, 1024, 18
    f2, f3 = fmaps(C, H, W, W, 3)
    sl = int(N.lib().sa_shear_slice_size(W, W, 4))
    assert B * H * sl > LINE

    def run(R_):
        a, b = rep(f2, R_), rep(f3, R_)
        out = torch.zeros((R_ * H, sl), device=dev)
        N.call("sa_corr_volume_pyramid_sheared", a.data_ptr(), b.data_ptr(), R_, C, H, W, W, 4.0, None, None, 0.9, 4,
               out.data_ptr(), U.stream())
        return out
    one, out = run(1), run(B)
    assert_replicas(out, one, B, "sheared pyramid")
    assert float(one.abs().max()) > 0
    del out, one
    done("corr_volume_pyramid_sheared, 2.26e9 floats")


@pytest.mark.parametrize("form", ["rows", "strided", "strided sheared"])
def test_pyramid_from_volume_past_2_31_floats(form):
    """sa_corr_pyramid_from_volume(_strided)(_sheared): the output past 2^31 floats (the row layout's 36 x 32
    x 1024 rows of 1920, the sheared layout's 18 x 32 slices)."""
    need(16)
    H, W = 32, 1024
    B = 18 if "sheared" in form else 36
    vol = np.random.default_rng(4).standard_normal((1, 1, W, H, W)).astype(np.float32)   # [1, 1, W2, H, W1]

    def run(R_):
        if form == "rows":   # [R_, 1, H, W1, W2], rows contiguous along W2
            return ops.pyramid_from_volume(rep(np.ascontiguousarray(vol.transpose(0, 1, 3, 4, 2)), R_), 4)
        v = rep(vol, R_).permute(0, 1, 3, 4, 2)
        if form == "strided":
            return ops.pyramid_from_volume(v, 4)
        sl = int(N.lib().sa_shear_slice_size(W, W, 4))
        out = torch.zeros((R_ * H, sl), device=dev)
        N.call("sa_corr_pyramid_from_volume_strided_sheared", v.data_ptr(), R_, H, W, W, v.stride(0), v.stride(2),
               v.stride(4), 4, out.data_ptr(), U.stream())
        return out
    one, out = run(1), run(B)
    assert out.numel() > LINE
    assert_replicas(out, one, B, f"pyramid from volume ({form})")
    del out, one
    done(f"pyramid_from_volume {form}")


@pytest.mark.parametrize("B", [63, 64], ids=["63: feature map under 2 GiB - 64 B", "64: first past it"])
def test_corr_volume_on_both_sides_of_the_feature_map_line(B):
    """corr_volume.hip's dispatch on f2_bytes: C 256, H 32, W1 1024 is 2^25 bytes per image; 63 images stay
    below 2 GiB - 64 B (the buffer-resource kernel), 64 are the first past it (the pointer kernel).  One
    level, W2 = 64.  Replicas on bits; rows 0, the last and the middle one of replica 0 against float64."""
    need(6)
    C, H, W1, W2 = 256, 32, 1024, 64
    f2, f3 = fmaps(C, H, W1, W2, 5)
    assert (B * C * H * W1 * 4 < LINE - 64) == (B == 63)
    one = ops.corr_volume(rep(f2, 1), rep(f3, 1)) if B == 63 else None   # (one sample runs the 63-image kernel)
    out = ops.corr_volume(rep(f2, B), rep(f3, B))   # [B, H, W1, 1, W2]
    assert_replicas(out, one, B, f"corr_volume B {B}")
    rows = (0, H // 2, H - 1)
    ref = R.corr_volume(f2[:, :, list(rows)], f3[:, :, list(rows)])   # [1, 3, W1, W2]
    tol = 2e-6 * np.abs(ref).max() + 1e-6   # test_corr_volume_and_pyramid's
    for b in (0, B - 1):   # (the last image holds the rows furthest from the base)
        np.testing.assert_allclose(out[b][list(rows)][:, :, 0].cpu().numpy(), ref[0], atol=tol)
    del out, one
    done(f"corr_volume B {B}")


# ------------------------------------------------------------------------------------------ (b) lookup
def _lookup_inputs(H, W):
    g = torch.Generator(device=dev).manual_seed(H)
    vols = [torch.randn((1, H, W, W), generator=g, device=dev) for _ in range(2)]
    cx = torch.rand((1, 1, H, W), generator=g, device=dev) * (W + 40) - 20
    cx[0, 0, H - 1, W - 1] = 984.5   # level 3 (the row's last 128 floats): taps reach cells 127 and 128
    cx[0, 0, 0, 0] = -3.0            # the first pixel's taps reach before the buffer
    return vols, cx


@pytest.mark.parametrize("H", [273, 274], ids=["273: pyramid under 2 GiB - 64 B", "274: first past it"])
def test_lookup_on_both_sides_of_the_pyramid_line(H):
    """corr_lookup.hip's dispatch on the pyramid's bytes: W1 = W2 = 1024, 4 levels (7680 B per row), B = 1.
    H = 273 is 2,146,959,360 B, the largest the buffer-resource kernel takes; H = 274 is the first on the
    pointer kernel.  Two volumes in one launch.  sa_corr_lookup and sa_corr_lookup_conv1x1; rows 0, the
    last (which holds the pyramid's last floats and, at 274, the 2^31-byte line) and the middle one against the
    float64 restatement at the ops' own tolerances."""
    need(9)
    W, L, r = 1024, 4, 4
    vols, cx = _lookup_inputs(H, W)
    pyrs = [ops.pyramid_from_volume(v, L) for v in vols]
    nbytes = pyrs[0].numel() * 4
    assert pyrs[0].shape == (H * W, 1920) and (nbytes < LINE - 64) == (H == 273)
    rng = np.random.default_rng(6)
    wt = (rng.standard_normal((64, 36)) / 6).astype(np.float32)
    bias = rng.standard_normal(64).astype(np.float32)
    taps = ops.corr_lookup(pyrs[0], pyrs[1], W, L, r, cx)   # [1, 72, H, W]
    fused = ops.corr_lookup_conv1x1(pyrs[0], pyrs[1], W, L, r, cx, torch.from_numpy(wt.T.copy()).to(dev),
                                    torch.from_numpy(bias).to(dev))   # [2, 64, H, W]
    torch.cuda.synchronize()
    rows = [0, H // 2, H - 1]
    cxs = cx[:, 0, rows].cpu().numpy()
    for v in range(2):
        ref = R.corr_lookup(R.corr_pyramid(vols[v][:, rows].cpu().numpy(), L), cxs, r, L)   # [1, 36, 3, W]
        np.testing.assert_allclose(taps[:, 36 * v:36 * v + 36][:, :, rows].cpu().numpy(), ref, atol=TOL_LOOKUP)
        want = np.maximum(np.einsum("ok,bkhw->bohw", wt.astype(np.float64), ref) + bias[None, :, None, None], 0)
        np.testing.assert_allclose(fused[v:v + 1][:, :, rows].cpu().numpy(), want, atol=2e-5)   # test_lookup_fused_convc1's
    del taps, fused, pyrs, vols
    done(f"lookup H {H} ({nbytes} B per pyramid)")


def test_sheared_lookup_past_2_31_floats():
    """sa_corr_lookup_conv1x1_sheared on two sheared pyramids of [281 x 8, 957,952] = 2.15e9 floats each (W 500: the
    widest class sa_corr_shear_supported takes is 511, so the sheared lookup has no case beside the row layout's
    2 GiB dispatch at W2 = 1024; it has no such dispatch either)."""
    need(24)
    H, W, L, r, B = 8, 500, 4, 4, 281
    rng = np.random.default_rng(12)
    vols = [rng.standard_normal((1, H, W, W)).astype(np.float32) for _ in range(2)]
    cx1 = (rng.random((1, 1, H, W)) * (W + 40) - 20).astype(np.float32)
    wt = torch.from_numpy((rng.standard_normal((36, 64)) / 6).astype(np.float32)).to(dev)
    bias = torch.from_numpy(rng.standard_normal(64).astype(np.float32)).to(dev)

    def run(R_):
        assert ops.shear_supported(R_, H, W, W, L)
        sh = [ops.corr_pyramid_shear(ops.pyramid_from_volume(rep(v, R_), L), R_, H, W, W, L) for v in vols]
        if R_ == B:
            assert sh[0].numel() > LINE
        out = ops.corr_lookup_conv1x1_sheared(sh[0], sh[1], W, L, r, rep(cx1, R_), wt, bias)   # [2 R_, 64, H, W]
        return (out.view(R_, 2 * 64 * H * W),)
    replicated(run, B, "corr_lookup_conv1x1_sheared")


# -------------------------------------------------------------------------------- (b) volume-sized ops
@pytest.mark.parametrize("mode,n,H,B", [(0, 1000, 30, 72), (1, 250, 60, 573)], ids=["line kernels", "one pass"])
def test_softargmin_volume_past_2_31_floats(mode, n, H, B):
    """sa_softargmin_conf on a [B, n, H, n] volume (the model's layout, sj = 1) past 2^31 floats: the line
    kernels at n = 1000, the one-pass slice kernel at n = 250.  (Per-image sizes that do not divide 2^31: a
    wrapped offset cannot land on the same position of another replica.)"""
    need(10)
    vol = (np.random.default_rng(n).standard_normal((1, n, H, n)) * 4).astype(np.float32)
    assert B * n * H * n > LINE

    def run(R_):
        v = rep(vol, R_)
        N.lib().sa_softargmin_set_one_pass(mode)
        try:
            return ops.softargmin_conf(v, v, (n * H * n, n, 1, H * n), (R_, H, n, n))
        finally:
            N.lib().sa_softargmin_set_one_pass(1)
    one, out = run(1), run(B)
    for o, w, what in zip(out, one, ("disparity", "confidence")):
        assert_replicas(o, w, B, f"softargmin {what}")
    if n <= 300:   # the widths the op's own test and tolerance cover (test_softargmin_confidence_lines: up to 300)
        cf = R.estimate_left_confidence(vol.transpose(0, 2, 3, 1)[:, :1])   # row 0 of [1, H, W1, W2] -> [1, 1, 1, W1]
        np.testing.assert_allclose(out[1][B - 1, 0, 0].cpu().numpy(), cf[0, 0, 0], atol=TOL_SOFTARGMIN_CONF)
    del out, one
    done(f"softargmin_conf mode {mode}")


def test_volume_stage_past_2_31_floats():
    """sa_volume_peak, sa_volume_stage (roll inside a bin, then the truncation) and
    sa_volume_truncate_backward on a [72, 1, 30, 1000, 1000] volume."""
    need(18)
    H, W, B = 30, 1000, 72
    rng = np.random.default_rng(7)
    vol = rng.standard_normal((1, 1, H, W, W)).astype(np.float32)
    mde = rng.random((1, 1, H, W)).astype(np.float32)
    d, m = (rng.random((1, 1, H, W)) * 40).astype(np.float32), rng.random((1, 1, H, W)).astype(np.float32)

    def run(R_):
        v = rep(vol, R_)
        peak = ops.volume_peak(v)
        out = ops.volume_stage(v, "roll", rep(mde, R_), 4, 1, 5, trunc_disp=rep(d, R_), trunc_conf=rep(m, R_))
        ops.volume_truncate_backward(v, rep(d, R_), rep(m, R_), 0.9, out=v)   # in place: the volume is not needed again
        return peak, out, v
    one, out = run(1), run(B)
    assert out[1].numel() > LINE
    assert torch.equal(bits(out[0]), bits(one[0])) and float(out[0]) == float(vol.max())
    assert_replicas(out[1], one[1], B, "volume_stage")
    assert_replicas(out[2], one[2], B, "volume_truncate_backward")
    del out, one
    done("volume_peak / volume_stage / volume_truncate_backward")


# ------------------------------------------------------------------------------- (b) hourglass volumes
@pytest.mark.parametrize("kind", ["vol_apply", "conv3d", "conv3d stride 2", "conv3d_wd", "conv3d_mf"])
def test_hourglass_volume_past_2_31_floats(kind):
    """[287, 8, 60, 120, 130] = 2.15e9 floats into sa_vol_apply and the 8-channel 3x3x3 convs (the direct form at
    stride 1 and 2, the Winograd-along-D form, the split-f16 MFMA form), each with the producer's norm and
    LeakyReLU applied on load and its statistics partials on.  Per image 7.5e6 floats (no divisor of 2^31), far below the kernels'
    own gates: only the batch total crosses.  The MFMA form picks its planes per block from the batch size, so
    its one-sample run is not compared; its replicas are."""
    need(18)
    C, D, H, W, B = 8, 60, 120, 130, 287
    x1 = np.random.default_rng(10).standard_normal((1, C, D, H, W)).astype(np.float32)
    w = (np.random.default_rng(11).standard_normal((C, 27, 16 if "stride 2" in kind else C)) * 0.1).astype(np.float32)
    assert B * C * D * H * W > LINE

    def run(R_):
        norm = (torch.full((R_ * C,), 0.1, device=dev), torch.full((R_ * C,), 1.5, device=dev))
        v = ops.VolAct(rep(x1, R_), norm, act=True)
        wt = torch.from_numpy(w).to(dev)
        if kind == "vol_apply":
            return (ops.vol_apply(v).raw,)
        if kind == "conv3d":
            a = ops.conv3d(v, wt, C)
        elif kind == "conv3d stride 2":
            a = ops.conv3d(v, wt, 16, stride=2)
        elif kind == "conv3d_wd":
            a = ops.conv3d_wd(v, ops.conv3d_wd_weights(torch.from_numpy(w)).to(dev), C)
        else:
            a = ops.conv3d_mf(v, ops.conv3d_mf_weights(wt), C)
        return a.raw, a.norm[0], a.norm[1]   # the output and the statistics its blocks' partials give
    one = None if kind == "conv3d_mf" else run(1)
    out = run(B)
    for i, o in enumerate(out):
        assert_replicas(o, None if one is None else one[i], B, f"{kind} output {i}")
    assert float(out[0][0].abs().max()) > 0
    del out, one
    done(f"hourglass {kind}")


# ------------------------------------------------------------------------- (b) 2-D elementwise epilogues
def test_elementwise_past_2_31_floats():
    """sa_relu_copy, sa_norm_act (with a skip), sa_plane_stats and sa_gru_out on [538, 64, 120, 520] = 2.15e9
    floats.  The inputs are windows of one replicated buffer (they are only read), so the case holds the
    buffer and one output at a time."""
    need(18)
    C, H, W, B = 64, 120, 520, 538
    x1 = np.random.default_rng(8).standard_normal((1, C, H, W)).astype(np.float32)
    assert B * C * H * W > LINE

    def run(R_):
        """(name, output) one at a time: the caller is done with an output before the next overwrites it"""
        x = rep(x1, R_ + 2)[:R_]   # two more images behind the last: sa_gru_out reads 3 C planes from every image
        out = torch.empty_like(x)
        ops.relu_copy(x, out)
        yield "relu_copy", out
        aff = ops.Affine(*(torch.linspace(-1, 1, C, device=dev) * k for k in (0.1, 1.5, 0.2)))
        ops.norm_act(x, aff, "relu", skip=x, act_out="relu", out=out)
        yield "norm_act", out
        mean, rstd = ops.plane_stats(x)
        yield "plane_stats", torch.stack([mean.view(R_, C), rstd.view(R_, C)], 1)
        # h (= out) in place; xc [B, 3 C, H W], qh, cq and z are all read through x with batch stride C H W, so
        # image b's q planes are image b + 2's first C planes: the same values in every replica
        out.copy_(x)
        N.call("sa_gru_out", x.data_ptr(), C * H * W, None, x.data_ptr(), C * H * W, x.data_ptr(), C * H * W,
               x.data_ptr(), R_, C, H * W, out.data_ptr(), C * H * W, U.stream())
        yield "gru_out", out

    ones = {k: v.clone() for k, v in run(1)}
    for k, v in run(B):
        assert_replicas(v.contiguous(), ones[k], B, k)
    assert float(ones["relu_copy"].min()) == 0.0 and float(ones["gru_out"].abs().max()) > 0
    done("relu_copy / norm_act / plane_stats / gru_out")


def test_convex_upsample_mask_past_2_31_floats():
    """sa_convex_upsample and its backward: the mask [B, 144, 64, 128] past 2^31 floats at B = 1821."""
    need(20)
    H, W, f, B = 64, 128, 4, 1821
    rng = np.random.default_rng(9)
    flow = (rng.standard_normal((1, 1, H, W)) * 3).astype(np.float32)
    mask = rng.standard_normal((1, 9 * f * f, H, W)).astype(np.float32)
    g = rng.standard_normal((1, 1, f * H, f * W)).astype(np.float32)
    assert B * 144 * H * W > LINE

    def run(R_):
        fl, mk = rep(flow, R_), rep(mask, R_)
        up = ops.convex_upsample(fl, mk, f)
        gf, gm = ops.convex_upsample_backward(fl, mk, rep(g, R_), f)
        return up, gf, gm
    one, out = run(1), run(B)
    for o, w, what in zip(out, one, ("out", "grad_flow", "grad_mask")):
        assert_replicas(o, w, B, f"convex_upsample {what}")
    del out, one
    done("convex_upsample + backward")


# ------------------------------------------------------------------------------------- (a) far strides
# ------------------------------------------------------------- (b) further dense cases, one op per case
def replicated(run, B, label, one_sample=True):
    """run(R) -> tuple of outputs with R replicas; every replica on bits, replica 0 against the one-sample run
    unless the op picks its kernel or block shape from the batch size."""
    one = run(1) if one_sample else None
    out = run(B)
    for i, o in enumerate(out):
        assert_replicas(o, None if one is None else one[i], B, f"{label} output {i}")
    assert float(out[0].view(B, -1)[B - 1].abs().max()) > 0, f"{label}: the last replica is all zero"
    del out, one
    done(label)


def sample(seed, *shape, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def test_gru_zr_past_2_31_floats():
    """sa_gru_zr: z and rh [1076, 64, 120 x 260] = 2.15e9 floats each.  The five inputs are one sample read with
    batch stride 0 (every image reads the same planes), so the case holds the two outputs only."""
    need(18)
    C, HW, B = 64, 120 * 260, 1076
    xc, hzr, cz, cr, h = (torch.from_numpy(sample(20 + i, k * C, HW)).to(dev) for i, k in enumerate((3, 2, 1, 1, 1)))

    def run(R_):
        z, rh = torch.empty((R_, C, HW), device=dev), torch.empty((R_, C, HW), device=dev)
        N.call("sa_gru_zr", xc.data_ptr(), 0, None, hzr.data_ptr(), 0, cz.data_ptr(), cr.data_ptr(), 0, h.data_ptr(), 0,
               R_, C, HW, z.data_ptr(), rh.data_ptr(), U.stream())
        return z, rh
    assert B * C * HW > LINE
    replicated(run, B, "gru_zr")


@pytest.mark.parametrize("kind", ["conv2d_small", "conv_direct stem", "conv_direct_split stem"])
def test_stem_convs_past_2_31_floats(kind):
    """The 7x7 stems, Cin 2 or 3 -> 64: the output [1076, 64, 120, 260] = 2.15e9 floats."""
    need(10)
    H, W, B = 120, 260, 1076
    Cin = 2 if kind == "conv2d_small" else 3
    x1 = sample(30, 1, Cin, H, W)
    w = torch.from_numpy(sample(31, 64, Cin, 7, 7, scale=0.1)).to(dev)
    bias = torch.from_numpy(sample(32, 64)).to(dev)
    wg = None if Cin == 2 else ops.conv_direct_weights(w, 1, split="split" in kind)

    def run(R_):
        x = rep(x1, R_)
        out = torch.empty((R_, 64, H, W), device=dev)
        if Cin == 2:
            N.call("sa_conv2d_small", x.data_ptr(), x.stride(0), R_, Cin, H, W, w.data_ptr(), bias.data_ptr(), 64, 7, 1,
                   out.data_ptr(), out.stride(0), U.stream())
        else:
            N.call("sa_conv_direct_split" if "split" in kind else "sa_conv_direct", x.data_ptr(), x.stride(0), R_, Cin,
                   H, W, 7, 1, wg.data_ptr(), None, 64, out.data_ptr(), out.stride(0), None, 0, None, None, U.stream())
        return (out,)
    replicated(run, B, kind)


@pytest.mark.parametrize("kind", ["F(2x2)", "F(4x4) block shape 0", "F(4x4) block shape 6"])
def test_winograd_convs_past_2_31_floats(kind):
    """3x3 convs 8 -> 32 with bias and ReLU: the output [2152, 32, 120, 260] = 2.15e9 floats.  The block shapes are
    forced through the entry points (no launch heuristic), so the one-sample run takes the same kernel."""
    need(12)
    Cin, Cout, H, W, B = 8, 32, 120, 260, 2152
    x1 = sample(33, 1, Cin, H, W)
    Uw = ops.wino_weights(torch.from_numpy(sample(34, Cout, Cin, 3, 3, scale=0.1)).to(dev))
    bias = torch.from_numpy(sample(35, Cout)).to(dev)

    def run(R_):
        x = rep(x1, R_)
        out = torch.empty((R_, Cout, H, W), device=dev)
        if kind == "F(2x2)":
            N.call("sa_conv2d_k3_wino", x.data_ptr(), x.stride(0), R_, Cin, H, W, Uw.u2.data_ptr(), Cout,
                   bias.data_ptr(), 1, out.data_ptr(), out.stride(0), U.stream())
        else:
            shape = int(kind[-1])
            prob, _ = ops._wino_problem(x, Uw, bias, True, out=out, f4=True, split=shape == 6)
            arr, gates = (N.SaWinoProblem * 1)(prob), (N.SaGateEpilogue * 1)()
            N.call("sa_conv2d_k3_wino4_launch", 1, U.ctypes.addressof(arr), U.ctypes.addressof(gates), shape,
                   1 if shape == 6 else 0, U.stream())
        return (out,)
    assert B * Cout * H * W > LINE
    replicated(run, B, kind)


def test_mask_upsample_past_2_31_floats():
    """sa_mask_upsample: x [4303, 64, 60, 130] = 2.15e9 floats."""
    need(12)
    Cin, H, W, B = 64, 60, 130, 4303
    x1, fl1 = sample(36, 1, Cin, H, W), sample(37, 1, 1, H, W, scale=3.0)
    ws = ops.conv1x1_weights(torch.from_numpy(sample(38, 144, Cin, scale=0.1)).to(dev))
    bias = torch.from_numpy(sample(39, 144)).to(dev)
    assert B * Cin * H * W > LINE
    replicated(lambda R_: (ops.mask_upsample(rep(x1, R_), ws, bias, 0.25, rep(fl1, R_)),), B, "mask_upsample")


@pytest.mark.parametrize("kind", ["lookup", "pyramid", "volume"])
def test_corr_backward_past_2_31_floats(kind):
    """The plug-in's adjoints: a gradient pyramid [144 x 8 x 1000 rows, 1876] = 2.16e9 floats written by
    sa_corr_lookup_backward and read by sa_corr_pyramid_backward; a gradient volume [269, 8, 1000, 1000] =
    2.15e9 floats read by sa_corr_volume_backward."""
    need(16)
    H, W, L, r = 8, 1000, 4, 4
    rs = ops.pyramid_geometry(W, L)[0]
    if kind == "lookup":
        B = 144
        g1 = sample(40, 1, L * (2 * r + 1), H, W)
        cx1 = (np.random.default_rng(41).random((1, 1, H, W)) * (W + 40) - 20).astype(np.float32)
        assert B * H * W * rs > LINE
        replicated(lambda R_: (ops.corr_lookup_backward(rep(g1, R_), rep(cx1, R_), W, L, r),), B, "corr_lookup_backward")
    elif kind == "pyramid":
        B = 144
        g1 = sample(42, 1, H * W, rs)
        assert B * H * W * rs > LINE
        replicated(lambda R_: (ops.pyramid_backward(rep(g1, R_).view(R_ * H * W, rs), W, L),), B, "pyramid_backward")
    else:
        B, C = 269, 16
        g1, f2, f3 = sample(43, 1, H, W, W), sample(44, 1, C, H, W), sample(45, 1, C, H, W)
        assert B * H * W * W > LINE
        replicated(lambda R_: tuple(ops.corr_volume_backward(rep(g1, R_), rep(f2, R_), rep(f3, R_))), B,
                   "corr_volume_backward")


def test_softargmin_backward_past_2_31_floats():
    """sa_softargmin_conf_backward on a disparity volume [4295, 8, 250, 250] = 2.15e9 floats (sk = 1, the layout
    training passes): the volume and its gradient."""
    need(18)
    H, n, B = 8, 250, 4295
    v1, gl1, gr1 = sample(46, 1, H, n, n, scale=4.0), sample(47, 1, H, n), sample(48, 1, H, n)

    def run(R_):
        v, gl, gr = rep(v1, R_), rep(gl1, R_), rep(gr1, R_)
        gd = torch.empty_like(v)
        ws = torch.empty(int(N.lib().sa_softargmin_conf_backward_ws_size(R_, H, n, n)) // 8 + 1, dtype=torch.float64,
                         device=dev)
        N.call("sa_softargmin_conf_backward", v.data_ptr(), None, R_, H, n, n, H * n * n, n * n, n, 1, gl.data_ptr(),
               gr.data_ptr(), None, None, gd.data_ptr(), None, ws.data_ptr(), U.stream())
        return (gd,)
    assert B * H * n * n > LINE
    replicated(run, B, "softargmin_conf_backward")


HG = (60, 120, 130)   # D, H, W of the hourglass cases: 936,000 cells, no divisor of 2^31


def _norm(R_, C):
    return torch.full((R_ * C,), 0.1, device=dev), torch.full((R_ * C,), 1.5, device=dev)


@pytest.mark.parametrize("kind", ["close", "conv3d_s2mf", "pointwise", "pointwise_upcat", "trilinear_up_adjoint",
                                  "pointwise_backward", "k3_backward_weight"])
def test_hourglass_training_ops_past_2_31_floats(kind):
    """The hourglass's remaining volume ops with B*C*D*H*W past 2^31 floats at their smallest built channel
    counts (8 channels at B 287, 16 at B 144): the close (statistics and backward, the upstream gradient aliased
    onto x so the case holds two volumes), the stride-2 MFMA conv, the 1x1x1 convs of the joins, the up-sampling
    adjoint and the two weight gradients.  A weight gradient sums over the batch, so it has no replica: with B
    identical samples it is B times the one-sample gradient up to rounding.  Both kernels add at most R products
    in fp32 (R = 32 for the 1x1x1 conv, 1024 for the 3x3x3 one) before the sums go on in float64, and how the
    cells are cut into such runs may follow the batch size; the upstream gradient is x itself, so the largest
    element is a sum of squares and bounds every element's sum of |products|.  Bound, relative to the largest
    element: R 2^-24 for the runs plus 2 x 2^-24 for the two roundings to fp32.  A misread sample changes the
    result by about 1 / B = 3.5e-3."""
    need(22)
    D, H, W = HG
    if kind == "close":
        B, C = 287, 8
        x1 = sample(50, 1, C, D, H, W)

        def run(R_):
            x = rep(x1, R_)
            mean, rstd = ops.volume_close_stats(x)
            dx, _, _ = ops.volume_close_backward(x, x, mean, rstd)
            return dx, mean.view(R_, C), rstd.view(R_, C)
        replicated(run, B, "volume_close stats + backward")
    elif kind == "conv3d_s2mf":
        B, C = 144, 16
        x1 = sample(51, 1, C, D, H, W)
        w = torch.from_numpy(sample(52, C, 27, 32, scale=0.1)).to(dev)
        table = ops.conv3d_s2mf_weights(w)
        assert table is not None

        def run(R_):
            a = ops.conv3d_s2(ops.VolAct(rep(x1, R_), _norm(R_, C), act=True), w, table, 32)
            return a.raw, a.norm[0].view(R_, 32), a.norm[1].view(R_, 32)
        replicated(run, B, "conv3d_s2mf")
    elif kind == "pointwise":
        B, C = 144, 16
        x1 = sample(53, 1, C, D, H, W)
        w = torch.from_numpy(sample(54, C, 8, scale=0.3)).to(dev)
        replicated(lambda R_: (ops.conv3d_pointwise(ops.VolAct(rep(x1, R_), _norm(R_, C), act=True), w, 8),), B,
                   "conv3d_pointwise")
    elif kind == "pointwise_upcat":
        B = 287
        a1, u1 = sample(55, 1, 8, D, H, W), sample(56, 1, 16, D // 2, H // 2, W // 2)
        wa, wu = (torch.from_numpy(sample(57 + i, c, 8, scale=0.3)).to(dev) for i, c in enumerate((8, 16)))

        def run(R_):
            o = ops.conv3d_pointwise_upcat(ops.VolAct(rep(a1, R_)), ops.VolAct(rep(u1, R_), _norm(R_, 16), act=True), wa,
                                           wu, 8)
            return o.raw, o.norm[0].view(R_, 8), o.norm[1].view(R_, 8)
        replicated(run, B, "conv3d_pointwise_upcat")
    elif kind == "trilinear_up_adjoint":
        B = 287
        g1 = sample(59, 1, 8, D, H, W)
        replicated(lambda R_: (ops.trilinear_up_adjoint(rep(g1, R_), (D // 2, H // 2, W // 2)),), B,
                   "trilinear_up_adjoint")
    else:
        B, C = 287, 8
        x1 = sample(60, 1, C, D, H, W)
        w = torch.from_numpy(sample(61, C, C, scale=0.3)).to(dev)

        def grads(R_):
            x = rep(x1, R_)   # the upstream gradient is x itself: one volume held
            if kind == "pointwise_backward":
                return ops.conv3d_pointwise_backward(x, x, w)
            return None, ops.conv3d_k3_backward_weight(x, x)
        dx1, dw1 = grads(1)
        dx, dw = grads(B)
        if dx is not None:
            assert_replicas(dx, dx1, B, "conv3d_pointwise_backward dx")
        want, got = dw1.double() * B, dw.double()
        err = float((got - want).abs().max() / want.abs().max())
        print(f"[large offsets] {kind}: dw(B) against B dw(1), largest relative difference {err:.3e}")
        bound = ((32 if kind == "pointwise_backward" else 1024) + 2) * 2.0 ** -24
        assert err <= bound, (err, bound)
        del dx, dx1, dw, dw1
        done(kind)


# (last in the module: the arenas live from the first far row to the module's end, and no dense case runs beside them)
@pytest.fixture(scope="module")
def arenas():
    need(17)   # two arenas of 2^31 + 64 + 2^22 floats
    a = U.Arena(dev), U.Arena(dev)
    yield a
    del a
    done("far-stride arenas released")


def test_far_rows_are_the_tables():
    assert {w for k, w in U.TABLE.values() if k == "far"} <= set(U.FAR_ROWS)


@pytest.mark.parametrize("name", list(U.FAR_ROWS))
def test_far_batch_stride(name, arenas):
    _, params, fn = U.FAR_ROWS[name]

    def run(far):
        p = U.Placer(far, *arenas, device=dev)
        outs = fn(p)
        torch.cuda.synchronize()
        assert p.seen == set(far), f"{name}: the far stride did not reach {set(far) - p.seen}"
        return [bits(o).clone() for o in outs]

    want = run(())
    sets = [(q,) for q in params] + ([params] if len(params) > 1 else [])
    for far in sets:
        got = run(far)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and torch.equal(g, w), \
                f"{name}: output {i} with the far stride on {', '.join(far)} differs from the dense call " \
                f"in {int((g != w).sum())} of {w.numel()} elements"


def test_far_views_are_far(arenas):
    p = U.Placer(("x",), *arenas, device=dev)
    v = p.inp("x", torch.ones(2, 3, 5))
    assert v.stride(0) == U.FAR and v[1].data_ptr() - v[0].data_ptr() == 4 * U.FAR > 1 << 33
    assert p.out("x", (2, 7)).stride(0) == U.FAR

"""The 2^31 / 2^30 / 65535 size gates of the C ABI that no other *_abi_cpu.py file pins, without a GPU: the
first refused value returns SA_E_ARG (-1) and sa_last_error() names the limit.  Validation happens before any
HIP call (a launch without a device would return SA_E_LAUNCH, -2, instead), so any non-null fake pointers do.
The gates this file's pull request tightened are pinned at their new values: sa_conv_direct's image size in
bytes, the sheared lookup's pixel count, sa_softargmin_conf's and sa_corr_pyramid_from_volume's grids."""
import ctypes

import pytest

from stereoanywhere_amd import _native as N

A, B_, C_, D_, E_, F_, G_ = (1 << 20), (1 << 24), (1 << 28), (1 << 30), (1 << 34), (1 << 36), (1 << 38)   # 16-byte aligned
T30, T31 = 1 << 30, 1 << 31


def L():
    return N.lib()


def _job(**kw):
    """sa_resample_multi of one pool2x job with these fields changed"""
    jobs = (N.SaResampleJob * 1)()
    fields = dict(kind=0, in_=A, in_bs=64, in_pitch=8, B=1, C=1, H=8, W=8, Ho=4, Wo=4, out=B_, out_bs=16, out_pitch=4)
    fields.update(kw)
    for k, v in fields.items():
        setattr(jobs[0], k, v)
    return L().sa_resample_multi(1, ctypes.addressof(jobs), None)


# (label, call, message); every call must return -1 and leave the message
CASES = [
    # gru.hip: one grid row per image (65535), a plane's flat index in 32 bits
    ("gru_zr B", lambda: L().sa_gru_zr(A, 64, None, B_, 64, C_, D_, 64, E_, 64, 65536, 1, 8, F_, G_, None), b"sa_gru_zr: empty shape or B 65536 above 65535"),
    ("gru_zr plane", lambda: L().sa_gru_zr(A, T31, None, B_, T31, C_, D_, T31, E_, T31, 1, 1 << 11, 1 << 20, F_, G_, None),
     b"sa_gru_zr: plane too large (C*HW = 2147483648 must be below 2^31)"),
    ("gru_out B", lambda: L().sa_gru_out(A, 64, None, B_, 64, C_, 64, D_, 65536, 1, 8, E_, 64, None), b"sa_gru_out: empty shape or B 65536 above 65535"),
    ("gru_out plane", lambda: L().sa_gru_out_split(A, T31, None, B_, None, T31, C_, T31, D_, 1, 1 << 11, 1 << 20, E_, T31, None),
     b"sa_gru_out: plane too large (C*HW = 2147483648 must be below 2^31)"),
    ("relu_copy B", lambda: L().sa_relu_copy(A, 8, 65536, 1, 8, B_, 8, None), b"sa_relu_copy: bad shape (B 65536 must be 1..65535"),
    ("relu_copy plane", lambda: L().sa_relu_copy(A, T31, 1, 1 << 11, 1 << 20, B_, T31, None), b"C*HW = 2147483648 below 2^31)"),
    ("flow_update B", lambda: L().sa_flow_update(A, None, 0, 65536, 2, 4, B_, 16, None, 0, None), b"sa_flow_update: bad shape (B 65536 must be 1..65535"),
    ("flow_update plane", lambda: L().sa_flow_update(A, None, 0, 1, 1 << 16, 1 << 15, B_, T31 * 2, None, 0, None),
     b"H*W = 2147483648 below 2^31)"),
    ("pool2x planes", lambda: L().sa_pool2x(A, 64, 256, 256, 8, 8, B_, 16, None), b"sa_pool2x: bad shape (B*C = 65536 planes must be 1..65535)"),
    ("pool2x plane", lambda: L().sa_pool2x_p(A, T31, 1 << 15, 1, 1, 1 << 16, 8, B_, T31, 4, None), b"sa_pool2x: plane too large"),
    ("pool2x flat index", lambda: L().sa_pool2x(A, 1 << 28, 1, 1, 1 << 13, 1 << 15, B_, 1 << 26, None),
     b"sa_pool2x: output plane shape unsupported (plane too large)"),
    ("interp planes", lambda: L().sa_interp_bilinear_ac(A, 64, 256, 256, 8, 8, 4, 4, B_, 16, None),
     b"sa_interp_bilinear_ac: bad shape (B*C = 65536 planes must be 1..65535)"),
    ("interp plane", lambda: L().sa_interp_bilinear_ac_p(A, T31, 1 << 15, 1, 1, 1 << 16, 8, 4, 4, B_, 16, 4, None),
     b"sa_interp_bilinear_ac: plane too large"),
    ("resample_multi planes", lambda: _job(B=256, C=256),
     b"sa_resample_multi: bad shape (B*C = 65536 planes must be 1..65535)"),
    ("resample_multi plane", lambda: _job(H=1 << 16, in_pitch=1 << 15, Ho=1 << 15),
     b"sa_resample_multi: plane too large"),
    # conv2d_small.hip, norm_act.hip
    ("narrow B", lambda: L().sa_conv2d_k3_narrow(A, 64, 65536, 8, 2, 4, B_, None, 2, C_, 16, None),
     b"sa_conv2d_k3_narrow: bad shape (B 65536 must be 1..65535"),
    ("narrow plane", lambda: L().sa_conv2d_k3_narrow(A, E_, 1, 8, 1 << 16, 1 << 15, B_, None, 2, C_, E_, None),
     b"sa_conv2d_k3_narrow: plane too large (H*W = 2147483648 must be below 2^31)"),
    ("norm_act planes", lambda: L().sa_norm_act(A, 64, 256, 256, 8, None, None, None, 0, 0, None, 0, None, None, None, 0, 0, 0,
                                                B_, 64, None), b"sa_norm_act: too many planes"),
    # corr_volume.hip
    ("corr_volume_pyramid grid", lambda: L().sa_corr_volume_pyramid(A, B_, 1 << 16, 16, 1 << 15, 4, 4, 4.0, None, None, 0.9, 1,
                                                                     C_, 4, None), b"sa_corr_volume_pyramid: grid too large"),
    ("pyramid_from_volume grid", lambda: L().sa_corr_pyramid_from_volume(A, (1 << 33) - 3, 8, 8, 1, B_, 8, None),
     b"sa_corr_pyramid_from_volume: grid too large (rows = 8589934589 must be below 2^33 - 3)"),
    ("pyramid_from_volume_strided B", lambda: L().sa_corr_pyramid_from_volume_strided(A, 65536, 2, 8, 8, 128, 8, 16, 1, B_, 8, None),
     b"sa_corr_pyramid_from_volume_strided: bad shape (B 65536 and H 2 must be 1..65535)"),
    ("pyramid_from_volume_strided H", lambda: L().sa_corr_pyramid_from_volume_strided(A, 2, 65536, 8, 8, 1 << 24, 8, 1 << 20, 1, B_, 8,
                                                                                       None), b"sa_corr_pyramid_from_volume_strided: bad shape (B 2 and H 65536 must be 1..65535)"),
    ("pyramid_from_volume_strided_sheared B", lambda: L().sa_corr_pyramid_from_volume_strided_sheared(A, 65536, 2, 8, 8, 128, 8, 16, 1,
                                                                                                      B_, None),
     b"sa_corr_pyramid_from_volume_strided_sheared: bad shape (B 65536 and H 2 must be 1..65535)"),
    # corr_shear.hip (2^31 - 2 = 42966 x 49981: inside the old gate, outside the new one)
    ("pyramid_shear rows", lambda: L().sa_corr_pyramid_shear(A, 120, 256, 256, 64, 64, 4, B_, None),
     b"sa_corr_pyramid_shear: more than 65535 image rows"),
    ("sheared lookup pixels", lambda: L().sa_corr_lookup_conv1x1_sheared(A, None, 64, 4, 4, B_, T31, 42966, 1, 49981, C_, D_, 64, E_, None),
     b"sa_corr_lookup_conv1x1_sheared: too many pixels (B*H*W1 = 2147483646 must be below 2^31 - 255)"),
    # softargmin.hip
    ("softargmin grid", lambda: L().sa_softargmin_conf(A, None, 1 << 15, 1 << 10, 64, 64, 1 << 22, 64, 1, 1 << 16, B_, C_, None, None,
                                                       1 << 16, None),
     b"sa_softargmin_conf: grid too large (B*H*max(W1, W2) = 2147483648 lines must be below 2^31)"),
    # corr_backward.hip
    ("lookup_backward row stride", lambda: L().sa_corr_lookup_backward(A, 10000, B_, 100, 1, 4, 8, 64, 4, 4, C_, T31, None),
     b"sa_corr_lookup_backward: row_stride out of range"),
    ("pyramid_backward grid", lambda: L().sa_corr_pyramid_backward(A, 1 << 39, 4, 4, 1, B_, 4, None),
     b"sa_corr_pyramid_backward: grid too large"),
    ("volume_backward grid", lambda: L().sa_corr_volume_backward(A, 4, B_, C_, 1 << 16, 16, 1 << 15, 4, 4, 4.0, D_, E_, None),
     b"sa_corr_volume_backward: grid too large"),
    # conv_direct.hip: 3 x 178956970 x 1 x 4 = 2147483640 bytes, the first at or past 2^31 - 16
    ("conv_direct image", lambda: L().sa_conv_direct(A, T31, 1, 3, 178956970, 1, 7, 1, B_, None, 64, C_, E_, None, 0, None, None, None),
     b"sa_conv_direct: image too large (Cin*H*W*4 = 2147483640 bytes must be below 2^31 - 16)"),
    ("conv_direct_split image", lambda: L().sa_conv_direct_split(A, T31, 1, 3, 178956970, 1, 7, 1, B_, None, 64, C_, E_, None, 0, None,
                                                                 None, None), b"sa_conv_direct: image too large"),
    # the hourglass convs
    ("conv3d plane", lambda: L().sa_conv3d(A, 1, 8, 1 << 11, 1 << 10, 1 << 10, 1, B_, 8, None, None, 0, 0.01, None, None, C_, None, None),
     b"sa_conv3d: a channel plane must hold < 2^31 voxels"),
    ("conv3d_wd bytes", lambda: L().sa_conv3d_wd(A, 1, 8, 1 << 9, 1 << 10, 1 << 10, B_, 8, None, None, 0, 0.01, None, None, C_, None, None),
     b"sa_conv3d_wd: a channel volume must hold < 2^31 bytes"),
    ("conv3d_s2mf cells", lambda: L().sa_conv3d_s2mf(A, 1, 1 << 10, 1 << 10, 1 << 10, B_, C_, D_, 0.01, None, None, E_, None, None),
     b"sa_conv3d_s2mf: volume too large (the split range needs D*H*W < 2^30)"),
    ("conv3d_s2mf image", lambda: L().sa_conv3d_s2mf(A, 1, 1 << 9, 1 << 9, 1 << 9, B_, C_, D_, 0.01, None, None, E_, None, None),
     b"sa_conv3d_s2mf: volume too large"),
    ("conv3d_onehot plane", lambda: L().sa_conv3d_onehot(A, B_, 1, 8, 1 << 11, 1 << 10, 1 << 10, 2, 1.73, C_, 16, D_, None, None),
     b"sa_conv3d_onehot: a channel plane must hold < 2^31 voxels"),
    # the 1x1 family and the flow head
    ("mask_upsample plane", lambda: L().sa_mask_upsample(A, F_, 1, 64, 1 << 14, 1 << 13, B_, None, 1.0, C_, D_, F_, None),
     b"sa_mask_upsample: plane too large"),
    ("mask_upsample blocks", lambda: L().sa_mask_upsample(A, 64 << 12, 1 << 30, 64, 64, 64, B_, None, 1.0, C_, D_, 16 << 12, None),
     b"sa_mask_upsample: too many blocks"),
    ("conv1x1 blocks", lambda: L().sa_conv1x1(A, 32 << 12, 1 << 30, 32, 64, 64, B_, 32, None, 1.0, C_, 32 << 12, None), b"sa_conv1x1: too many blocks"),
    ("flow_head_reduce N", lambda: L().sa_flow_head_reduce(A, 65536, 32, 8, 16, B_, C_, None, 0, None, 0, None),
     b"sa_flow_head_reduce: bad shape (N 65536 must be 1..65535"),
]


@pytest.mark.parametrize("label,call,message", CASES, ids=[c[0] for c in CASES])
def test_first_refused_value(label, call, message):
    rc = call()
    assert rc == -1, f"{label}: returned {rc} ({L().sa_last_error()!r}); -2 would mean a launch was attempted"
    assert message in L().sa_last_error(), L().sa_last_error()


def test_shear_supported_at_the_pixel_line():
    """Host only.  2^31 pixels are refused and 2^31 - 1024 taken, as before; the kernels' 32-bit pixel index of
    the last block's idle lanes moves the line to 2^31 - 255."""
    q = L().sa_corr_shear_supported
    assert q(32768, 1, 65536, 64, 4) == 0                      # 2^31
    assert q(49, 1024, 42799, 64, 4) == 1                      # 2^31 - 1024 = 1024 x 49 x 127 x 337
    assert 49 * 1024 * 42799 == T31 - 1024
    assert q(12032, 1, 178481, 64, 4) == 1 and 12032 * 178481 == T31 - 256   # the last value taken
    assert q(42966, 1, 49981, 64, 4) == 0 and 42966 * 49981 == T31 - 2       # inside the old gate
    assert q(65536, 1, 8, 64, 4) == 0 and q(65535, 1, 8, 64, 4) == 1         # one grid z-slice per image row
    assert q(1, 8, 520, 512, 4) == 0 and q(1, 8, 520, 511, 4) == 1           # the LDS tile of the widest level


def test_the_model_takes_the_row_layout_at_2_31_pixels(monkeypatch):
    """The layout dispatch (StereoAnywhere._pyramid_route, called by the forward; the issue names corr.py, the
    decision is the model's) with the library's query wrapped, not replaced, and nothing allocated: at
    B*H*W1 = 2^31 the route is the row layout, HipCorrBlock1D.from_features is asked for it, calls the row
    producer and has no sheared buffer; at 2^31 - 1024 the sheared route is taken.  The query's arguments are
    the geometry, unchanged."""
    import types

    from stereoanywhere_amd import corr, model, ops
    real, seen, made = N.lib(), [], []

    class Lib:
        def __getattr__(self, name):
            return getattr(real, name)

        def sa_corr_shear_supported(self, *a):
            seen.append(a)
            return real.sa_corr_shear_supported(*a)
    monkeypatch.setattr(N, "lib", lambda: Lib())
    monkeypatch.setattr(ops, "corr_volume_pyramid", lambda *a, **k: made.append("rows") or "row pyramid")
    monkeypatch.setattr(ops, "corr_volume_pyramid_sheared", lambda *a, **k: made.append("sheared") or "sheared pyramid")
    me = types.SimpleNamespace(opts=model.ScheduleOptions(), args=types.SimpleNamespace(corr_levels=4))
    assert me.opts.sheared_lookup and me.opts.sheared_producers
    for B, H4, W4 in ((32768, 1, 65536), (49, 1024, 42799)):
        # the model's volumes are square (W2 = W1): these widths are far past the 511-wide LDS tile, so the
        # library says no for that reason alone; what is checked is that its answer is obeyed and what it is asked
        assert model.StereoAnywhere._pyramid_route(me, B, H4, W4) == (False, False)
        assert seen[-1] == (B, H4, W4, W4, 4)
    # the pixel line itself: the same geometries asked at a width the sheared kernels take
    monkeypatch.setattr(ops, "shear_supported", lambda B, H, W1, W2, L=4: bool(Lib().sa_corr_shear_supported(B, H, W1, 64, L)))
    for (B, H4, W4), want in (((32768, 1, 65536), False), ((49, 1024, 42799), True)):
        big, direct = model.StereoAnywhere._pyramid_route(me, B, H4, W4)
        assert (big, direct) == (want, want), (B, H4, W4)
        assert seen[-1] == (B, H4, W4, 64, 4)
        f2 = types.SimpleNamespace(shape=(B, 16, H4, W4))
        blk = corr.HipCorrBlock1D.from_features(f2, f2, 4, 4, sheared=direct)
        assert made[-1] == ("sheared" if want else "rows")
        assert (blk.sheared is None) == (not want) and (blk.pyramid is None) == want
    # an answer ignored or inverted would show: the route follows the query alone
    monkeypatch.setattr(ops, "shear_supported", lambda *a: False)
    assert model.StereoAnywhere._pyramid_route(me, 1, 16, 256) == (False, False)
    monkeypatch.setattr(ops, "shear_supported", lambda *a: True)
    assert model.StereoAnywhere._pyramid_route(me, 1, 16, 256) == (True, True)


def test_the_flow_head_epilogue_is_refused_on_the_small_block_shape():
    """The hole in the far-stride table's F(4x4) matrix: gate mode 3 on block shape 2 is an argument error."""
    prob = (N.SaWinoProblem * 1)()
    gate = (N.SaGateEpilogue * 1)()
    q = prob[0]
    q.in_, q.in_bs, q.N, q.Cin, q.H, q.W, q.U, q.Cout, q.relu, q.out = A, 32 * 128, 1, 32, 8, 16, B_, 32, 1, C_
    gate[0].mode, gate[0].head_w, gate[0].head_part, gate[0].head_part_bs = 3, D_, C_, 1 << 20
    call = L().sa_conv2d_k3_wino4_launch
    assert call(1, ctypes.addressof(prob), ctypes.addressof(gate), 2, 0, None) == -1
    assert b"the 8-wave 32-channel shape (block_shape 0, 6 or 7)" in L().sa_last_error(), L().sa_last_error()

"""Replica, rerun, dirty-memory and two-stream bit-equality of the HIP ops (tests/invariance_util.py).

Every case replicates one seeded sample along the batch and asks, on bits: do identical inputs in
different blocks give identical results (P1), does the same call give the same result three times (P2),
whatever the destinations and the allocator's free blocks held before (P3: 0xFFFFFFFF words, zeros,
0xFFFFFFFF), and, where the op keeps process-global state or a multi-launch workspace, on two streams at
once (P4).  None of that says anything about accuracy, so each case also compares out[0] with the
restatement and the tolerance of the op's own test: it calls the op it claims to, on inputs where it works.

Shapes are the smallest at which the named machinery is engaged, taken from the ops' own tests.  The
one-block-per-sample kernels (weighted_lsq*) run 512 replicas: one launch is 512 trials of the same race.
"""
import numpy as np
import pytest
import torch

import lsq_lrc_ref as lsq_ref
from invariance_util import Case, PoisonDidNotTake, check_poison, poison_free_memory, run_case
from oracle import ops_ref as R
from stereoanywhere_amd import _native as N, ops

pytestmark = pytest.mark.gpu
dev = "cuda"
f32 = np.float32


def c(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def close(got, want, **tol):
    np.testing.assert_allclose(c(got) if isinstance(got, torch.Tensor) else got, want, **tol)


CASES = []


def case(name, **kw):
    def add(build):
        parts = build()   # (inputs, call, oracle[, dict of Case's optional hooks])
        CASES.append(Case(name, *parts[:3], **(parts[3] if len(parts) > 3 else {}), **kw))
        return build
    return add


# ------------------------------------------------------------------------------------ weighted LSQ
def lsq_sample(kind):
    """(mde, disp, conf) [1, n] of the four LSQ samples.
    a: n 8192, every disparity in [20, 20.24): one 15-bit key bin (0.25 wide in [16, 32)), so all 8192
       keys are pooled, eight per thread, and every term of the sums goes through the pooled-key pass;
    b: n 65280, test_weighted_lsq_zero_heavy's sample 0 at zfrac 0.2 (the zero bin; the model's n);
    c: n 17 (less than a wave);
    d: n 70001 (more than 64 keys per thread: past them the kernel streams and tests every key instead
       of revisiting the ones it marked), test_weighted_lsq_quantile_band_vs_oracle's sample 0."""
    if kind == "a":
        rng = np.random.default_rng(8192)
        n = 8192
        d = (20 + 0.24 * rng.random((1, n))).astype(f32)
        assert d.min() >= 20 and d.max() < 20.24
        assert len(set((d.view(np.uint32) >> 17).ravel().tolist())) == 1   # one bin of the top 15 bits
        m = rng.random((1, n)).astype(f32)
    elif kind == "b":
        n, zfrac = 65280, 0.2
        rng = np.random.default_rng(int(zfrac * 1e4))
        m = rng.random((2, n)).astype(f32)
        d = (40 * m + 3 + rng.standard_normal((2, n))).astype(f32)
        nz = int(round(zfrac * n))
        d[:, :nz] = -rng.random(nz).astype(f32)
        d[1, nz:nz + 50] = f32(1e-42)
        perm = rng.permutation(n)
        m, d = m[:1, perm].copy(), d[:1, perm].copy()
    else:
        n = 17 if kind == "c" else 70001
        rng = np.random.default_rng(n)
        m = rng.random((1, n)).astype(f32)
        d = (40 * m + 3 + rng.standard_normal((1, n))).astype(f32)
        d[:, : n // 7] = -1.0
    cf = np.random.default_rng(n + 1).random((1, n)).astype(f32)
    return m, d, cf


def lsq_band_keeps(d):
    lo, hi, keep = lsq_ref.band(torch.from_numpy(d[0]))
    return float(keep.float().mean())


def lsq_oracle_scale_shift(m, d, cf, sc, sh):
    rsc, rsh = R.weighted_lsq(m, d, cf)
    close(sc[:1], rsc, rtol=1e-5, atol=1e-5)
    close(sh[:1], rsh, rtol=1e-5, atol=1e-4)


def lsq_oracle_record(m, d, cf, rec):
    """test_weighted_lsq_record_and_partial_requests' check of the record: fp32 products, fp64 sums.
    The band is the oracle's (ops_ref.torch_quantile: at::lerp without contraction, as the kernel has
    it; torch's CPU lerp may contract a + w (b - a) into an fma, one ulp away at n = 17)."""
    r = c(rec)[0]
    y = np.maximum(d[0], 0)
    lo, hi = R.torch_quantile(y, 0.2), R.torch_quantile(y, 0.9)
    assert r[3] == float(lo) and r[4] == float(hi) and r[5] == 0.0
    k = (lo <= y) & (y <= hi)
    a, wt = np.abs(m[0].astype(np.float64))[k], (0.9 * np.abs(cf[0].astype(np.float64)) + 0.1)[k]
    want = np.array([(wt * a * a).sum(), (wt * a).sum(), wt.sum()])
    assert np.abs(r[:3] - want).max() <= 1e-6 * want.max()


def lsq_case(kind, form):
    def build():
        m, d, cf = lsq_sample(kind)
        if kind == "a":
            assert lsq_band_keeps(d) > 0.5   # more than half of the pooled keys add terms

        def inputs(rep):
            return rep(m), rep(d), rep(cf)

        def call(inp, dests):
            if form == "stats":
                return ops.weighted_lsq_stats(*inp)
            return ops.weighted_lsq(*inp, single_block=form == "one_block")

        def oracle(inp, outs):
            lsq_oracle_scale_shift(m, d, cf, outs[0], outs[1])
            if form == "stats":
                lsq_oracle_record(m, d, cf, outs[2])
        return inputs, call, oracle
    return build


for _kind in "abcd":
    for _form in ("one_block", "grid", "stats"):
        case(f"weighted_lsq[{_kind}-{_form}]", R=512, streams=True)(lsq_case(_kind, _form))


def lsq_backward_case(n, kind):
    def build():
        m, d, cf = (x[:1] for x in lsq_ref.lsq_inputs(n, kind))
        rng = np.random.default_rng(n + 1)
        gs, gt = rng.standard_normal(1).astype(f32), rng.standard_normal(1).astype(f32)

        def inputs(rep):
            tm, td, tc = rep(m), rep(d), rep(cf)
            return (tm, td, tc) + tuple(ops.weighted_lsq_stats(tm, td, tc)) + (rep(gs), rep(gt))

        def call(inp, dests):
            return ops.weighted_lsq_backward(*inp)

        def oracle(inp, outs):
            w64 = lsq_ref.weighted_lsq_grads(m, d, cf, gs, gt, torch.float64)
            w32 = lsq_ref.weighted_lsq_grads(m, d, cf, gs, gt, torch.float32)
            for a, x64, x32 in zip(outs, w64, w32):   # test_weighted_lsq_backward's yardstick
                got = c(a)[:1].astype(np.float64)
                assert np.isfinite(got).all() and np.abs(got - x64).max() <= 4 * np.abs(x32 - x64).max()
        return inputs, call, oracle
    return build


case("weighted_lsq_backward[594-random]", R=512)(lsq_backward_case(594, "random"))
case("weighted_lsq_backward[4320-ties]", R=512)(lsq_backward_case(4320, "ties"))


# ------------------------------------------------------------------------------------- cost volume
# ragged groups; W2 > 256 (split k blocks / 256-wide chunks)
CV_SHAPES = [(256, 3, 37, 45), (64, 2, 65, 300)]


def by_sample(t, B):
    """[B * rows, cols] (or [B * n, ...]) -> [B, ...]"""
    return t.reshape(B, -1, *t.shape[1:])


def used_columns(pyr, W2, L=4):
    _, offs, wids = ops.pyramid_geometry(W2, L)
    return pyr[:, :offs[-1] + wids[-1]]   # the row's padding to 4 floats is never written


def fmaps(C, H, W1, W2):
    rng = np.random.default_rng(C + H + W1 + W2)
    return rng.standard_normal((1, C, H, W1)).astype(f32), rng.standard_normal((1, C, H, W2)).astype(f32)


def corr_volume_case(C, H, W1, W2, what):
    def build():
        f2, f3 = fmaps(C, H, W1, W2)
        ref = R.corr_volume(f2, f3)
        tol = 2e-6 * np.abs(ref).max() + 1e-6   # test_corr_volume_and_pyramid's

        def inputs(rep):
            return rep(f2), rep(f3)

        def call(inp, dests):
            B = inp[0].shape[0]
            if what == "volume":
                return (ops.corr_volume(*inp),)
            return (by_sample(used_columns(ops.corr_volume_pyramid(*inp, 4), W2), B),)

        def oracle(inp, outs):
            if what == "volume":
                close(outs[0][:1, :, :, 0], ref, atol=tol)
                return
            _, offs, wids = ops.pyramid_geometry(W2, 4)
            got = c(outs[0])[0].reshape(H, W1, -1)
            for o, w, rv in zip(offs, wids, R.corr_pyramid(ref, 4)):
                np.testing.assert_allclose(got[None, ..., o:o + w], rv, atol=tol)
        return inputs, call, oracle
    return build


def truncated_pyramid_case(C, H, W):
    def build():
        f2, f3 = fmaps(C, H, W, W)
        rng = np.random.default_rng(W)
        d, m = (rng.random((1, 1, H, W)) * 40).astype(f32), rng.random((1, 1, H, W)).astype(f32)
        ref = R.truncate_volume(d, m, 0.9) * R.corr_volume(f2, f3)
        tol = 2e-6 * np.abs(ref).max() + 1e-6   # test_truncated_pyramid's

        def inputs(rep):
            return rep(f2), rep(f3), rep(d), rep(m)

        def call(inp, dests):
            f2, f3, d, m = inp
            return (by_sample(used_columns(ops.corr_volume_pyramid(f2, f3, 4, d, m, 0.9), W), f2.shape[0]),)

        def oracle(inp, outs):
            _, offs, wids = ops.pyramid_geometry(W, 4)
            got = c(outs[0])[0].reshape(H, W, -1)
            for o, w, rv in zip(offs, wids, R.corr_pyramid(ref.astype(f32), 4)):
                np.testing.assert_allclose(got[None, ..., o:o + w], rv, atol=tol)
        return inputs, call, oracle
    return build


def pyramid_from_volume_case(H, W1, W2, strided):
    def build():
        vol = np.random.default_rng(W1 + W2).standard_normal((1, 1, W2, H, W1)).astype(f32)   # the hourglass layout

        def inputs(rep):
            v = rep(vol)
            return (v.permute(0, 1, 3, 4, 2) if strided else v.permute(0, 1, 3, 4, 2).contiguous(),)

        def call(inp, dests):
            return (by_sample(used_columns(ops.pyramid_from_volume(inp[0], 4), W2), inp[0].shape[0]),)

        def oracle(inp, outs):
            _, offs, wids = ops.pyramid_geometry(W2, 4)
            got = c(outs[0])[0]
            rows = vol[0, 0].transpose(1, 2, 0).reshape(H * W1, W2)
            for o, w, lv in zip(offs, wids, R.corr_pyramid(rows, 4)[:4]):
                np.testing.assert_allclose(got[:, o:o + w], lv, atol=1e-6)   # test_pyramid_from_strided_volume's
        return inputs, call, oracle
    return build


def sheared_cells(sh, B, W1, W2):
    import test_gpu_ops as gpu_ops   # the level cells of a sheared pyramid; other entries are never read
    return by_sample(gpu_ops._sheared_valid_cells(sh, W1, W2), B)


def sheared_case(C, H, W1, W2, what):
    """The three producers of the sheared layout against the oracle's pyramid levels, cell by cell."""
    def build():
        f2, f3 = fmaps(C, H, W1, W2)
        vol = np.random.default_rng(W1 * W2).standard_normal((1, 1, W2, H, W1)).astype(f32)

        def inputs(rep):
            if what == "volume":
                return rep(f2), rep(f3)
            view = rep(vol).permute(0, 1, 3, 4, 2)
            return (view,) if what == "from_volume" else (view, ops.pyramid_from_volume(view, 4))

        def call(inp, dests):
            B = inp[0].shape[0]
            if what == "volume":
                sh = ops.corr_volume_pyramid_sheared(*inp, 4)
            elif what == "from_volume":
                sh = ops.pyramid_from_volume_sheared(inp[0], 4)
            else:
                sh = ops.corr_pyramid_shear(inp[1], B, H, W1, W2)
            assert sh is not None, "the sheared producer refused the geometry"
            return (sheared_cells(sh, B, W1, W2),)

        def oracle(inp, outs):
            # cell (e, j) of level l holds the row layout's k = (j >> l) - e + width_l - 1 of pixel j
            # (test_lookup_sheared_bit_exact); the levels are the oracle's, at the row-layout cases' tolerances
            if what == "volume":
                ref = R.corr_volume(f2, f3)
                levels, tol = R.corr_pyramid(ref, 4), 2e-6 * np.abs(ref).max() + 1e-6
            else:
                levels, tol = R.corr_pyramid(vol[0, 0].transpose(1, 2, 0).reshape(H * W1, W2), 4)[:4], 1e-6
            _, _, wids = ops.pyramid_geometry(W2, 4)
            cols = []
            for l in range(4):
                lv = np.asarray(levels[l]).reshape(H, W1, wids[l])
                E = wids[l] + ((W1 - 1) >> l)
                e = np.arange(E).reshape(E, 1)
                j = np.broadcast_to(np.arange(W1).reshape(1, W1), (E, W1))
                k = (j >> l) - e + wids[l] - 1
                ok = (k >= 0) & (k < wids[l])
                cols.append(lv[:, j[ok], k[ok]])
            want = np.concatenate(cols, 1)
            assert want.size == H * W1 * sum(wids)
            close(outs[0][0], want, atol=tol)
        return inputs, call, oracle
    return build


for _C, _H, _W1, _W2 in CV_SHAPES:
    _s = f"{_C}x{_H}x{_W1}x{_W2}"
    case(f"corr_volume[{_s}]")(corr_volume_case(_C, _H, _W1, _W2, "volume"))
    case(f"corr_volume_pyramid[{_s}]")(corr_volume_case(_C, _H, _W1, _W2, "pyramid"))
    case(f"pyramid_from_volume[contiguous-{_H}x{_W1}x{_W2}]")(pyramid_from_volume_case(_H, _W1, _W2, False))
    case(f"corr_pyramid_shear[{_H}x{_W1}x{_W2}]")(sheared_case(_C, _H, _W1, _W2, "shear"))
# the strided view and the sheared producers need W1 % 4 == 0 (W2 % 4 and C % 16 too for the volume)
for _C, _H, _W1, _W2 in [(256, 3, 36, 44), (64, 2, 64, 300)]:
    _s = f"{_C}x{_H}x{_W1}x{_W2}"
    case(f"pyramid_from_volume[strided-{_H}x{_W1}x{_W2}]")(pyramid_from_volume_case(_H, _W1, _W2, True))
    case(f"corr_volume_pyramid_sheared[{_s}]")(sheared_case(_C, _H, _W1, _W2, "volume"))
    case(f"pyramid_from_volume_sheared[{_H}x{_W1}x{_W2}]")(sheared_case(_C, _H, _W1, _W2, "from_volume"))
case("corr_volume_pyramid[truncated-256x3x45]")(truncated_pyramid_case(256, 3, 45))
case("corr_volume_pyramid[truncated-64x2x300]")(truncated_pyramid_case(64, 2, 300))


# ------------------------------------------------------------------------------------------ lookup
def lookup_case(what, L=4, r=4):
    """H 5, W 72; coordinates from -20 to W + 20, so edge taps are present."""
    def build():
        rng = np.random.default_rng(6 + L + r)
        H, W = 5, 72
        K = L * (2 * r + 1)
        va, vb = (rng.standard_normal((1, H, W, W)).astype(f32) for _ in range(2))
        cx = (rng.random((1, 1, H, W)) * (W + 40) - 20).astype(f32)
        assert cx.min() < 0 and cx.max() > W
        wt = (rng.standard_normal((64, K)) / 6).astype(f32)
        bias = rng.standard_normal(64).astype(f32)
        two = what != "lookup1"

        def inputs(rep):
            B = rep(cx).shape[0]
            pa, pb = (ops.pyramid_from_volume(rep(v), L) for v in (va, vb))
            if what == "sheared":
                pa, pb = (ops.corr_pyramid_shear(p, B, H, W, W, L) for p in (pa, pb))
            return pa, pb, rep(cx), torch.from_numpy(wt.T.copy()).to(dev), torch.from_numpy(bias).to(dev)

        def call(inp, dests):
            pa, pb, x, w, b = inp
            if what in ("lookup1", "lookup2"):
                return (ops.corr_lookup(pa, pb if two else None, W, L, r, x),)
            fn = ops.corr_lookup_conv1x1_sheared if what == "sheared" else ops.corr_lookup_conv1x1
            out = fn(pa, pb, W, L, r, x, w, b)   # [B * 2, 64, H, W], sample 2 b + v
            return (out.view(x.shape[0], 2, 64, H, W),)

        def oracle(inp, outs):
            taps = [R.corr_lookup(R.corr_pyramid(v, L), cx[:, 0], r, L) for v in (va, vb)]   # [1, K, H, W]
            if what in ("lookup1", "lookup2"):
                close(outs[0][:1], np.concatenate(taps[:2 if two else 1], 1), atol=1e-5)
                return
            for v in range(2):   # test_lookup_fused_convc1's
                ref = np.maximum(np.einsum("ok,bkhw->bohw", wt.astype(np.float64), taps[v]) + bias[None, :, None, None], 0)
                close(outs[0][:1, v], ref, atol=2e-5)
        return inputs, call, oracle
    return build


case("corr_lookup[one volume]")(lookup_case("lookup1"))
case("corr_lookup[two volumes]")(lookup_case("lookup2"))
case("corr_lookup_conv1x1")(lookup_case("fused"))
case("corr_lookup_conv1x1_sheared")(lookup_case("sheared"))
case("corr_lookup_conv1x1[3 levels, radius 2]")(lookup_case("fused", 3, 2))   # the tap-folding kernel
case("corr_lookup_conv1x1_sheared[3 levels, radius 2]")(lookup_case("sheared", 3, 2))


# -------------------------------------------------------------------------------------- regression
def softargmin_case(n, layout, mode):
    """_softargmin_lines of test_gpu_ops.py with one sample: H 3, two volumes that are channel views of
    one tensor; mode: sa_softargmin_set_one_pass (0 per-line kernels, 1 one-pass, 2 its 16-byte rows)."""
    def build():
        H = 3
        vols = (np.random.default_rng(n).standard_normal((1, 2, H, n, n)) * 4).astype(f32)   # [1,2,H,W1,W2]

        def inputs(rep):
            if layout == "reference":
                return (rep(vols),)
            return (rep(vols.transpose(0, 1, 4, 2, 3).copy()),)   # [B,2,W2,H,W1]

        def call(inp, dests):
            t = inp[0]
            strides = (2 * H * n * n, n * n, n, 1) if layout == "reference" else (2 * n * H * n, n, 1, H * n)
            N.lib().sa_softargmin_set_one_pass(mode)
            try:
                return tuple(ops.softargmin_conf(t[:, 0], t[:, 1], strides, (t.shape[0], H, n, n)))
            finally:
                N.lib().sa_softargmin_set_one_pass(1)

        def oracle(inp, outs):
            d, cf = outs
            vd, vc = vols[:, 0], vols[:, 1]
            close(d[:1, 0:1], R.estimate_left_disparity(vd), atol=5e-4)
            close(d[:1, 1:2], R.estimate_right_disparity(vd), atol=5e-4)
            close(cf[:1, 0:1], R.estimate_left_confidence(vc), atol=2e-6)
            close(cf[:1, 1:2], R.estimate_right_confidence(vc), atol=2e-6)
        return inputs, call, oracle
    return build


for _n in (64, 300):
    case(f"softargmin_conf[reference-{_n}]")(softargmin_case(_n, "reference", 1))
    for _mode in (0, 1, 2):
        case(f"softargmin_conf[native-{_n}-mode {_mode}]")(softargmin_case(_n, "native", _mode))


def softlrc_case(joint, conf, W=64):
    def build():
        H = 3
        d2, d3 = (x[:1] for x in lsq_ref.lrc_inputs(2, H, W, float(W), seed=100 * H + W))
        rng = np.random.default_rng(W)
        c2, c3 = (rng.random(d2.shape).astype(f32) for _ in range(2))

        def inputs(rep):
            if joint:
                return (rep(np.concatenate([d2, d3], 1)), rep(np.concatenate([c2, c3], 1)) if conf else None)
            return (rep(d2), rep(d3)) + ((rep(c2), rep(c3)) if conf else (None, None))

        def call(inp, dests):
            if joint:
                out = ops.softlrc_joint(*inp, 1.0)
                return out[:, :1], out[:, 1:]
            return tuple(ops.softlrc(*inp, 1.0))

        def oracle(inp, outs):
            s2, s3 = R.softlrc(d2, d3, 1.0)
            if conf:
                s2, s3 = c2 * s2, c3 * s3
            # test_softlrc's 2e-6 at W 64.  At W 300 the sample coordinate x -+ d is a float of size W, and
            # kernel and oracle may round its few operations differently: up to 4 ulp(W) in the bilinear
            # weight, times the largest step between neighbouring pixels of the sampled map, through
            # softplus (slope <= 1) and the division by log(1 + e) = 1.31
            tol = [2e-6, 2e-6]
            if W > 64:
                for k, other in enumerate((d3, d2)):
                    tol[k] += 4 * float(np.spacing(f32(W))) * float(np.abs(np.diff(other, axis=-1)).max()) / 1.31
            close(outs[0][:1], s2, atol=tol[0])
            close(outs[1][:1], s3, atol=tol[1])
        return inputs, call, oracle
    return build


for _W in (64, 300):
    case(f"softlrc_joint[{_W}]")(softlrc_case(True, False, _W))
    case(f"softlrc_joint[conf {_W}]")(softlrc_case(True, True, _W))
    case(f"softlrc[conf {_W}]")(softlrc_case(False, True, _W))
    case(f"softlrc[no conf {_W}]")(softlrc_case(False, False, _W))


def convex_upsample_case(misaligned):
    """7 x 13, the mask a channel slice of a larger buffer; the output aligned (the per-pixel kernel)
    or one float off 16 bytes (the per-output kernel), as test_convex_upsample_pixel_kernel_bit_exact."""
    def build():
        H, W = 7, 13
        rng = np.random.default_rng(H * W)
        flow = (rng.standard_normal((1, 1, H, W)) * 5).astype(f32)
        big = (rng.standard_normal((1, 150, H, W)) * 3).astype(f32)

        def inputs(rep):
            return rep(flow), rep(big)[:, 3:147]

        def dests(inp):
            return (torch.empty(inp[0].shape[0] * 16 * H * W + 4, device=dev),)

        def call(inp, dests):
            fl, mask = inp
            B, off = fl.shape[0], 1 if misaligned else 0
            out = dests[0][off:off + B * 16 * H * W].view(B, 1, 4 * H, 4 * W)
            assert out.data_ptr() % 16 == 4 * off
            return (ops.convex_upsample(fl, mask, 4, out=out),)

        def oracle(inp, outs):
            close(outs[0][:1], R.convex_upflow(flow, big[:, 3:147]), atol=1e-5)   # test_convex_upsample's
        return inputs, call, oracle, dict(dests=dests)
    return build


case("convex_upsample[aligned]")(convex_upsample_case(False))
case("convex_upsample[misaligned]")(convex_upsample_case(True))


# ---------------------------------------------------------------------------------- 3 x 3 convs
import contextlib   # noqa: E402

import torch.nn.functional as F   # noqa: E402


@contextlib.contextmanager
def conv_mode(mode):
    """The module switches test_gpu_wino.py sets with monkeypatch: "f2" the F(2x2) kernel; F(4x4) whatever
    the size with fp32 products ("fp32"), the split kernel ("split") or its single-f16 form ("mixed")."""
    saved = ops._WINO4, ops.W4_SPLIT, ops._WINO4_MIN_BLOCKS
    ops._WINO4, ops.W4_SPLIT, ops._WINO4_MIN_BLOCKS = mode != "f2", mode in ("split", "mixed"), 0
    try:
        with ops.mixed_precision(mode == "mixed"):
            yield
    finally:
        ops._WINO4, ops.W4_SPLIT, ops._WINO4_MIN_BLOCKS = saved


SHAPE_OF_MODE = {"fp32": 0, "split": 6, "mixed": 7}


def conv_ref(mode, x, w, bias=None):
    """The 3x3 conv an epilogue case's expected values are built from, in float64 on the CPU: F.conv2d,
    or in the mixed mode the plain mixed conv's own output (pinned to its restatement by the plain
    cases), as tests/test_gpu_wino_mixed.py builds the epilogue instances' expected values."""
    if mode != "mixed":
        return F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), padding=1)
    with conv_mode(mode):
        (y,) = ops.conv2d_k3_multi(dict(x=x.float().to(dev).contiguous(), U=ops.wino_weights(w.to(dev).contiguous()),
                                        bias=None if bias is None else bias.to(dev)))
    return y.double().cpu()


def redo_blocks():
    n = int(N.lib().sa_split_redo_blocks(1))   # reads and resets the range guard's redo counter
    assert n >= 0
    return n


def conv_check(got, ref64, mode):
    """test_wino4_matches_conv2d's bound (split and fp32 products: 1e-4 max, 1e-5 RMS of the output's
    RMS, floor 1), test_wino_matches_conv2d's for F(2x2); the mixed mode's against its restatement is
    conv_check_mixed."""
    ref = ref64.float()
    scale = max(float(ref.pow(2).mean().sqrt()), 1.0)
    err_max, err_rms = float((got - ref).abs().max()), float((got - ref).pow(2).mean().sqrt())
    assert torch.isfinite(got).all()
    if mode == "f2":
        assert err_max < 2e-4 * scale and err_rms < 2e-5 * scale, (err_max, err_rms)
    else:
        assert err_max < 1e-4 * scale and err_rms < 1e-5 * scale, (err_max, err_rms)


def conv_check_mixed(got, x, w, bias, relu):
    """test_mixed_matches_restatement's: RMS(gpu - restatement) <= 0.25 E, 0.75 E <= RMS(gpu - fp64) <= 1.25 E."""
    from mixed_ref import rms, wino4_mixed
    from test_split_numerics_cpu import direct
    xn, wn = x.cpu().numpy()[0], w.cpu().numpy()
    rest, f64 = wino4_mixed(xn, wn), direct(xn, wn)
    if bias is not None:
        bn = bias.cpu().numpy()[:, None, None]
        rest, f64 = rest + bn.astype(f32), f64 + bn.astype(np.float64)
    if relu:
        rest, f64 = np.maximum(rest, 0.0), np.maximum(f64, 0.0)
    g, E = got.cpu().numpy(), rms(rest - f64)
    assert np.isfinite(g).all() and E > 0
    assert rms(g - rest) <= 0.25 * E and 0.75 * E <= rms(g - f64) <= 1.25 * E, (rms(g - rest), rms(g - f64), E)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def conv3x3_case(mode, Cin, Cout, H, W, variant="plain"):
    """variant: "plain" (bias, ReLU, statistics), "affine" (the producer's scale, shift and ReLU on load),
    "small" (F(4x4)'s small block shape), "guard" (a patch of the input times 3e3: the split kernels'
    range guard fires and the blocks run again on scaled inputs; the redo counter is process-global)."""
    def build():
        x = rnd(1, Cin, H, W, seed=Cin + 1)
        w = rnd(Cout, Cin, 3, 3, seed=Cout + 1) / (3 * Cin ** 0.5)
        b = rnd(Cout, seed=8)
        s, t = rnd(Cin, seed=9).abs() + 0.5, rnd(Cin, seed=10)
        if variant == "guard":
            x[0, :, 2:6, W // 2:W // 2 + 12] *= 3e3
        stats = variant in ("plain", "small")
        relu = variant == "plain"

        def inputs(rep):
            with conv_mode(mode):
                U = ops.wino_weights(w.to(dev))
            assert (U.u4s is not None) == (mode in ("split", "mixed"))
            return rep(x), U, b.to(dev), ops.Affine(None, s.to(dev), t.to(dev))

        def call(inp, dests):
            xs, U, bias, aff = inp
            p = dict(x=xs, U=U, bias=bias, relu=relu, stats=stats)
            if variant == "affine":
                p.update(in_aff=aff, in_act="relu")
            ops.W4_SHAPE_LAUNCHES.clear()
            with conv_mode(mode):
                (res,) = ops.conv2d_k3_multi(p, small_blocks=variant == "small")
            if mode != "f2":   # the launch ran the kernel the case names
                assert set(ops.W4_SHAPE_LAUNCHES) == {2 if variant == "small" else SHAPE_OF_MODE[mode]}, ops.W4_SHAPE_LAUNCHES
            return (res[0],) + tuple(v.view(xs.shape[0], Cout) for v in res[1]) if stats else (res,)

        def oracle(inp, outs):
            xd, wd, bd = x.double(), w.double(), b.double()
            if variant == "affine":
                xd = torch.relu(xd * s.double()[:, None, None] + t.double()[:, None, None])
            ref = F.conv2d(xd, wd, bd, padding=1)
            ref = torch.relu(ref) if relu else ref
            got = outs[0][:1].cpu()
            if variant == "guard" and mode == "split":   # test_wino4_split_range_guard's: 1e-5 of max |y|
                assert torch.isfinite(got).all()
                assert float((got - ref.float()).abs().max()) < 1e-5 * float(ref.abs().max())
            elif variant == "guard":
                assert torch.isfinite(got).all()
                assert float((got - ref.float()).abs().mean() / ref.abs().mean()) < 5e-3
            elif mode == "mixed" and variant == "plain":
                conv_check_mixed(got, x, w, b, relu)
            elif mode == "mixed":   # test_mixed_input_transform's: the mode's own error from fp32, no more
                rel = float((got - ref.float()).abs().mean() / ref.abs().mean())
                assert 2e-4 < rel < 5e-3, rel
            else:
                conv_check(got, ref, mode)
            if stats:   # test_wino4_small_block_shape's
                torch.testing.assert_close(outs[1][:1].cpu(), got.mean(dim=(2, 3)), atol=1e-5, rtol=1e-5)
                torch.testing.assert_close(outs[2][:1].cpu(), (got.var(dim=(2, 3), unbiased=False) + 1e-5).rsqrt(),
                                           atol=1e-4, rtol=1e-4)

        def guard_fired(inp):   # around the first poisoned launch (the counter is read and reset)
            assert redo_blocks() > 0, "the range guard did not fire"
        hooks = dict(before=lambda inp: redo_blocks(), after=guard_fired) if variant == "guard" else {}
        return inputs, call, oracle, hooks
    return build


for _Cin, _Cout, _H, _W in [(16, 64, 9, 36), (64, 96, 17, 52)]:
    _s = f"{_Cin}->{_Cout} {_H}x{_W}"
    # (Cout % 64 == 0 runs two 32-channel groups per block, 96 one: both groupings of the F(2x2) kernel)
    case(f"conv2d_k3[F(2x2) {_s}]")(conv3x3_case("f2", _Cin, _Cout, _H, _W))
    for _mode in ("fp32", "split", "mixed"):
        case(f"conv2d_k3_multi[{_mode} {_s}]")(conv3x3_case(_mode, _Cin, _Cout, _H, _W))
        case(f"conv2d_k3_multi[{_mode} affine input {_s}]")(conv3x3_case(_mode, _Cin, _Cout, _H, _W, "affine"))
    case(f"conv2d_k3_multi[small blocks {_s}]")(conv3x3_case("fp32", _Cin, _Cout, _H, _W, "small"))
    for _mode in ("split", "mixed"):
        case(f"conv2d_k3_multi[{_mode} range guard {_s}]", streams=True)(conv3x3_case(_mode, _Cin, _Cout, _H, _W, "guard"))


# -------------------------------------------------------------------------------- update-loop glue
def gru_case(H, W, what):
    """C 128 at 9 x 13 (H W % 4 != 0: the scalar path) and 10 x 12 (float4); test_gru_gates_and_plumbing's
    inputs and tolerances.  gru_out works in place: every call starts from a copy of h."""
    def build():
        rng = np.random.default_rng(9)
        C = 128
        xc = rng.standard_normal((1, 3 * C, H, W)).astype(f32)
        hzr = rng.standard_normal((1, 2 * C, H, W)).astype(f32)
        ctx = rng.standard_normal((1, 3 * C, H, W)).astype(f32)
        h = np.tanh(rng.standard_normal((1, C, H, W))).astype(f32)
        qh, qa = (rng.standard_normal((1, C, H, W)).astype(f32) for _ in range(2))
        bx = rng.standard_normal(3 * C).astype(f32)
        use_bx = what.endswith("bx")
        b = bx[None, :, None, None] if use_bx else np.zeros((1, 3 * C, 1, 1), f32)
        zr = R.sigmoid(xc[:, :C] + b[:, :C] + hzr[:, :C] + ctx[:, :C])
        rr = R.sigmoid(xc[:, C:2 * C] + b[:, C:2 * C] + hzr[:, C:] + ctx[:, C:2 * C])
        q = np.tanh(xc[:, 2 * C:] + b[:, 2 * C:] + qh + ctx[:, 2 * C:])

        def inputs(rep):
            return dict(xc=rep(xc), hzr=rep(hzr), ctx=rep(ctx), h=rep(h), qh=rep(qh), qa=rep(qa), qb=rep(qh - qa),
                        z=rep(zr.astype(f32)), bx=torch.from_numpy(bx).to(dev) if use_bx else None)

        def dests(i):
            if what.startswith("zr"):
                return torch.empty_like(i["h"]), torch.empty_like(i["h"])
            return ()

        def call(i, dests):
            cx = i["ctx"]
            if what.startswith("zr"):
                ops.gru_zr(i["xc"], i["hzr"], cx[:, :C], cx[:, C:2 * C], i["h"], dests[0], dests[1], bx=i["bx"])
                return tuple(dests)
            hh = i["h"].clone()
            if what.startswith("out2"):
                ops.gru_out(i["xc"], i["qa"], cx[:, 2 * C:], i["z"], hh, bx=i["bx"], qh2=i["qb"])
            else:
                ops.gru_out(i["xc"], i["qh"], cx[:, 2 * C:], i["z"], hh, bx=i["bx"])
            return (hh,)

        def oracle(i, outs):
            if what.startswith("zr"):
                close(outs[0][:1], zr, atol=1e-6)
                close(outs[1][:1], rr * h, atol=1e-6)
            else:
                close(outs[0][:1], (1 - zr.astype(f32)) * h + zr.astype(f32) * q, atol=2e-6)
        return inputs, call, oracle, dict(dests=dests)
    return build


for _H, _W in ((9, 13), (10, 12)):
    for _what in ("zr", "zr-bx", "out", "out-bx", "out2", "out2-bx"):
        case(f"gru_{_what}[{_H}x{_W}]")(gru_case(_H, _W, _what))


def resample_case(what, hw_in, hw_out, pitch=0):
    """pool2x / interp / relu_copy into a channel slice of a wider buffer (as the update block does);
    pitch: pitched planes (row pitch W + pitch, pad columns zero and untouched)."""
    def build():
        C = 128 if max(hw_in) < 20 else 8
        (hi, wi), (ho, wo) = hw_in, hw_out
        x = np.random.default_rng(hi * wi).standard_normal((1, C, hi, wi)).astype(f32)

        def inputs(rep):
            xs = rep(x)
            if pitch:
                xs = F.pad(xs, (0, pitch))
            return (xs,)

        def dests(inp):
            return (torch.empty(inp[0].shape[0], 2 * C, ho, wo + pitch, device=dev),)

        def call(inp, dests):
            out = dests[0][:, C:]
            if pitch:
                out[..., wo:] = 0.0
            kw = dict(width=wi, out_width=wo) if pitch else {}
            if what == "pool2x":
                ops.pool2x(inp[0], out, **kw)
            elif what == "interp":
                ops.interp(inp[0], out, **kw)
            elif what == "multi":
                ops.resample_multi(("interp" if ho > hi else "pool", inp[0], out, *(kw.get(k) for k in ("width", "out_width"))))
            else:
                ops.relu_copy(inp[0], out)
            return (out,)

        def oracle(inp, outs):
            xs = inp[0][:1, ..., :wi]
            if what == "relu_copy":
                want = torch.relu(xs)
            elif ho < hi:
                want = F.avg_pool2d(xs, 3, 2, 1)
            else:
                want = F.interpolate(xs, (ho, wo), mode="bilinear", align_corners=True)
            torch.testing.assert_close(outs[0][:1, ..., :wo], want, atol=1e-6, rtol=0)
            if pitch:
                assert not outs[0][..., wo:].any()
        return inputs, call, oracle, dict(dests=dests)
    return build


case("pool2x[57x71->29x36]")(resample_case("pool2x", (57, 71), (29, 36)))
case("interp[29x36->57x71]")(resample_case("interp", (29, 36), (57, 71)))
case("interp[flat 5x6->9x13]")(resample_case("interp", (5, 6), (9, 13)))
case("interp[band 29x36->57x72]")(resample_case("interp", (29, 36), (57, 72)))
case("pool2x[pitched 57x71->29x36]")(resample_case("pool2x", (57, 71), (29, 36), pitch=4))
case("interp[pitched 29x36->57x71]")(resample_case("interp", (29, 36), (57, 71), pitch=4))
case("resample_multi[pool 57x71->29x36]")(resample_case("multi", (57, 71), (29, 36)))
case("resample_multi[interp 29x36->57x71]")(resample_case("multi", (29, 36), (57, 71)))
case("relu_copy[9x13]")(resample_case("relu_copy", (9, 13), (9, 13)))
case("relu_copy[10x12]")(resample_case("relu_copy", (10, 12), (10, 12)))


# ------------------------------------------------------------------------------------- mono volume
def mono_case(W, what):
    """H 6; W 25 (odd: the scalar path) and W 44; test_normals_masks_and_masked_volume's tolerances."""
    def build():
        H = 6
        rng = np.random.default_rng(W)
        m2, m3 = (rng.random((1, 1, H, W)).astype(f32) for _ in range(2))
        m2[0, 0, 0, :4] = [1.0, 0.0, 0.5, 0.375]   # 1.0 is in no bin; exact bin edges
        n2, n3 = R.estimate_normals(m2, 2.0), R.estimate_normals(m3, 2.0)
        w16 = torch.from_numpy((np.random.default_rng(3).standard_normal((8, 27, 16)) * 0.2).astype(f32))

        def inputs(rep):
            return rep(n2), rep(n3), rep(m2), rep(m3), w16.to(dev)

        def call(inp, dests):
            if what == "normals":
                return (ops.mono_normals(inp[2], 2.0),)
            if what == "volume":
                return (ops.mono_masked_volume(*inp[:4], 8, 1.73),)
            # the records of both views and their reader: the hourglass's stride-2 conv on the one-hot volume
            oh = ops.OneHotVolume(*inp[:4], 8, 1.73)
            a = ops.conv3d(oh, inp[4], 16, stride=2)
            B = inp[0].shape[0]
            return oh.rec_l, oh.rec_r, a.raw, a.norm[0].view(B, -1), a.norm[1].view(B, -1)

        def oracle(inp, outs):
            if what == "normals":
                close(outs[0][:1], n2, atol=1e-6)
            elif what == "volume":
                ref = R.masked_mono_volume(R.mono_corr_volume(n2, n3), R.generate_masks(m2), R.generate_masks(m3))
                close(outs[0][:1], ref.transpose(0, 1, 4, 2, 3), atol=1e-6)
            else:
                for rec, m in ((outs[0], m2), (outs[1], m3)):   # (n0, n1, n2, depth bin or -1)
                    masks = R.generate_masks(m)[0]   # [8, H, W]: half-open bins, 1.0 in none
                    np.testing.assert_array_equal(c(rec)[0, ..., 3], np.where(masks.any(0), masks.argmax(0), -1))
                # test_onehot_hourglass_readers_match_dense's: the same conv on the materialised volume
                one = [t[:1].contiguous() for t in inp[:4]]
                b = ops.conv3d(ops.VolAct(ops.mono_masked_volume(*one, 8, 1.73)), inp[4], 16, stride=2)
                torch.testing.assert_close(outs[2][:1], b.raw, atol=1e-5, rtol=1e-5)
                torch.testing.assert_close(outs[3][0], b.norm[0].flatten(), atol=1e-6, rtol=1e-5)
                torch.testing.assert_close(outs[4][0], b.norm[1].flatten(), atol=1e-6, rtol=1e-5)
        return inputs, call, oracle
    return build


for _W in (25, 44):
    for _what in ("normals", "volume", "records"):
        case(f"mono_{_what}[6x{_W}]")(mono_case(_W, _what))


# ---------------------------------------------------------------------------------------- backward
def softlrc_backward_case(H, W, field):
    """test_softlrc_backward's inputs (away from the kinks) and yardstick; the gather's fp64 workspace
    comes from torch.empty."""
    def build():
        d2, d3 = (x[:1] for x in lsq_ref.lrc_inputs(2, H, W, 3.0 if field == "small" else float(W), seed=100 * H + W))
        rng = np.random.default_rng(10 * H + W)
        c2, c3 = (rng.uniform(0.0, 1.0, d2.shape).astype(f32) for _ in range(2))
        g2, g3 = (rng.standard_normal(d2.shape).astype(f32) for _ in range(2))

        def inputs(rep):
            return tuple(rep(x) for x in (d2, d3, c2, c3, g2, g3))

        def call(inp, dests):
            return ops.softlrc_backward(*inp[:4], 1.0, inp[4], inp[5], True, True, True, True)

        def oracle(inp, outs):
            w64 = lsq_ref.softlrc_grads(d2, d3, c2, c3, 1.0, g2, g3, torch.float64)
            w32 = lsq_ref.softlrc_grads(d2, d3, c2, c3, 1.0, g2, g3, torch.float32)
            for a, x64, x32 in zip(outs, w64, w32):
                got = c(a)[:1].astype(np.float64)
                assert np.isfinite(got).all() and np.abs(got - x64).max() <= 4 * np.abs(x32 - x64).max()
        return inputs, call, oracle
    return build


case("softlrc_backward[5x7-small]")(softlrc_backward_case(5, 7, "small"))
case("softlrc_backward[3x65-wide]")(softlrc_backward_case(3, 65, "wide"))


# ----------------------------------------------------------------------------------- hourglass 3-D
@contextlib.contextmanager
def capture_partials():
    """Inside, ops.instnorm_finalize also records the partial sums it is handed ([b c][parts][2]
    float64, written by the conv's blocks): the cases compare them beside the finalized mean / rstd."""
    got, real = [], ops.instnorm_finalize

    def spy(partial, bc, parts, count, eps=1e-5):
        got.append(partial)
        return real(partial, bc, parts, count, eps)
    ops.instnorm_finalize = spy
    try:
        yield got
    finally:
        ops.instnorm_finalize = real


def rep_volact(v, rep):
    return ops.VolAct(rep(v.raw), None if v.norm is None else tuple(rep(t.view(1, -1)).reshape(-1) for t in v.norm),
                      v.act, None if v.gate is None else tuple(rep(g) for g in v.gate))


def with_stats(a, partials, B):
    return (a.raw,) + tuple(p.view(B, -1) for p in partials) + (a.norm[0].view(B, -1), a.norm[1].view(B, -1))


def hourglass_case(kind, cin, cout, shape, gated=False, stride=1):
    """One kernel of tests/test_gpu_hourglass_ref.py at its smallest shape past one tile, with that
    test's inputs (one sample), float64 reference and derived elementwise bound; statistics on."""
    def build():
        seed = cin + cout + sum(shape)
        nf = {"direct": (8 if cout <= 8 else 2 if cout >= 32 else 4) if stride == 1 else 2,
              "wd": 8 if cin == 8 else 4, "mf": 16 if cin == 8 else 8, "s2": 8, "pointwise": 0}[kind]

        def inputs(rep):
            import test_gpu_hourglass_ref as hg
            v, tx, mr = hg._input(cin, shape, seed, gate=gated, B=1)
            w = hg._weights(cin, cout, seed, k=1 if kind == "pointwise" else 27)
            i = dict(v=rep_volact(v, rep), tx=tx, mr=mr, w=w, wg=w.to(dev))
            if kind == "wd":
                i["w_wd"] = ops.conv3d_wd_weights(w).to(dev)
            if kind in ("mf", "s2"):
                i["table"] = (ops.conv3d_mf_weights if kind == "mf" else ops.conv3d_s2mf_weights)(w.to(dev))
                assert i["table"] is not None
            return i

        def call(i, dests):
            B = i["v"].raw.shape[0]
            with capture_partials() as parts:
                if kind == "direct":
                    a = ops.conv3d(i["v"], i["wg"], cout, stride=stride, slope=0.01)
                elif kind == "wd":
                    a = ops.conv3d_wd(i["v"], i["w_wd"], cout, slope=0.01)
                elif kind == "mf":
                    a = ops.conv3d_mf(i["v"], i["table"], cout, slope=0.01)
                elif kind == "s2":
                    a = ops.conv3d_s2(i["v"], i["wg"], i["table"], cout, slope=0.01)
                else:
                    return (ops.conv3d_pointwise(i["v"], i["wg"], cout, slope=0.01),)
            assert len(parts) == 1
            return with_stats(a, parts, B)

        def oracle(i, outs):
            import hourglass_ref as HG
            import test_gpu_hourglass_ref as hg
            tx, mr, w, U = i["tx"], i["mr"], i["w"], hg.U
            if kind == "pointwise":
                ref, mag = HG.pointwise(tx, w)
                bound = (cin + 6) * U * mag
            elif kind == "wd":
                ref, bound = HG.conv3(tx, w)[0], (9 * cin + 17) * U * hg._f43(tx, ops.conv3d_wd_weights(w), True)
            else:
                ref, mag = HG.conv3(tx, w, stride)
                bound = hg._split_bound(tx, mr, w, stride, mag) if kind in ("mf", "s2") else (27 * cin + 6) * U * mag
            hg._check(f"{kind} {cin}->{cout} {shape}", outs[0][:1], ref, bound)
            if kind != "pointwise":
                hg._check_stats(f"{kind} {cin}->{cout} {shape}", ops.VolAct(outs[0][:1], (outs[2][0], outs[3][0])), nf)
        return inputs, call, oracle
    return build


case("conv3d[stride 1, 8->8 9x5x63]")(hourglass_case("direct", 8, 8, (9, 5, 63)))
case("conv3d[stride 1, 16->16 gated 5x5x63]")(hourglass_case("direct", 16, 16, (5, 5, 63), gated=True))
case("conv3d[stride 2, 8->16 4x17x62]")(hourglass_case("direct", 8, 16, (4, 17, 62), stride=2))
case("conv3d_wd[8->8 3x5x63]")(hourglass_case("wd", 8, 8, (3, 5, 63)))
case("conv3d_wd[16->16 gated 5x3x63]")(hourglass_case("wd", 16, 16, (5, 3, 63), gated=True))
case("conv3d_mf[8->8 3x9x65]")(hourglass_case("mf", 8, 8, (3, 9, 65)))
case("conv3d_mf[16->16 3x5x65]")(hourglass_case("mf", 16, 16, (3, 5, 65)))
case("conv3d_s2[16->32 6x10x33]")(hourglass_case("s2", 16, 32, (6, 10, 33), stride=2))
case("conv3d_s2[16->32 gated 3x3x5]")(hourglass_case("s2", 16, 32, (3, 3, 5), gated=True, stride=2))
case("conv3d_pointwise[16->8 gated 3x5x7]")(hourglass_case("pointwise", 16, 8, (3, 5, 7), gated=True))
case("conv3d_pointwise[32->16 4x6x65]")(hourglass_case("pointwise", 32, 16, (4, 6, 65)))


def upcat_case(form, shape, low):
    """conv3d_pointwise_upcat <8, 8, raw a> and <16, 16, gated a> of test_conv3d_pointwise_upcat: two
    launches (the low-resolution product p is a torch.empty workspace of the op)."""
    def build():
        seed = sum(shape) + len(form)
        ca, cu, cout = (16, 32, 16) if form == "16x16 gated" else (8, 16, 8)

        def inputs(rep):
            import test_gpu_hourglass_ref as hg
            u, tu, _ = hg._input(cu, low, seed + 1, gate=True, B=1)
            a, ta, _ = hg._input(ca, shape, seed, norm=ca == 16, act=ca == 16, gate=ca == 16, B=1)
            wa, wu = hg._weights(ca, cout, seed, k=1), hg._weights(cu, cout, seed + 1, k=1)
            return dict(a=rep_volact(a, rep), u=rep_volact(u, rep), ta=ta, tu=tu, wa=wa, wu=wu,
                        wag=wa.to(dev), wug=wu.to(dev))

        def call(i, dests):
            with capture_partials() as parts:
                r = ops.conv3d_pointwise_upcat(i["a"], i["u"], i["wag"], i["wug"], cout, slope=0.01)
            return with_stats(r, parts, i["a"].raw.shape[0])

        def oracle(i, outs):
            import hourglass_ref as HG
            import test_gpu_hourglass_ref as hg
            ref, m = HG.upcat(i["ta"], i["tu"], i["wa"], i["wu"])
            hg._check(f"upcat {form}", outs[0][:1], ref, hg._upcat_bound(ca, cu, m))
            hg._check_stats(f"upcat {form}", ops.VolAct(outs[0][:1], (outs[2][0], outs[3][0])), 4)
        return inputs, call, oracle
    return build


case("conv3d_pointwise_upcat[8x8 raw 9x6x130]")(upcat_case("8x8 raw", (9, 6, 130), (5, 3, 65)))
case("conv3d_pointwise_upcat[16x16 gated 10x7x67]")(upcat_case("16x16 gated", (10, 7, 67), (3, 2, 20)))


# ------------------------------------------------------- F(4x4) epilogues, pitched planes, flow head
def gate_case(mode, pitch=0):
    """The GRU gate epilogues of test_wino4_gru_gate_epilogues / test_split5_gate_epilogues at 8 x 128
    (mode 1 needs whole 32-channel blocks of z and r), one launch each: mode 1 writes z and r*h beside a
    second, plain conv; mode 2 updates h in place (every call starts from a copy).  pitch: the planes
    pitched by 4 zero columns (W 124 of 128)."""
    def build():
        g = torch.Generator(device="cpu").manual_seed(42)
        hd, xd, H, P = 32, 16, 8, 128
        W = P - pitch

        def r(*s):
            t = torch.randn(*s, generator=g)
            if pitch and len(s) == 4:
                t[..., W:] = 0.0
            return t
        hxr, ctx = r(1, 2 * hd + xd, H, P), r(1, 3 * hd, H, P)
        wz, wr, wq = (r(hd, hd + xd, 3, 3) / (3 * (hd + xd) ** 0.5) for _ in range(3))
        bz, br, bq = r(hd), r(hd), r(hd)
        z0, qx0 = torch.sigmoid(r(1, hd, H, P)), r(1, hd, H, P)
        kw = dict(width=W) if pitch else {}

        def inputs(rep):
            with conv_mode(mode):
                Uzr = ops.wino_weights(torch.cat([wz, wr]).contiguous().to(dev))
                Uqx, Uqh = ops.wino_weights(wq[:, hd:].contiguous().to(dev)), ops.wino_weights(wq[:, :hd].contiguous().to(dev))
            return dict(hxr=rep(hxr), ctx=rep(ctx), z=rep(z0), qx=rep(qx0), Uzr=Uzr, Uqx=Uqx, Uqh=Uqh,
                        bzr=torch.cat([bz, br]).to(dev), bq=bq.to(dev))

        def dests(i):
            B = i["hxr"].shape[0]
            return tuple(torch.empty(B, hd, H, P, device=dev) for _ in range(3))

        def call(i, dests):
            z, qx, rh = dests
            if pitch:   # (the pad columns of pitched outputs are zero and stay zero)
                for t in dests:
                    t[..., W:] = 0.0
            hxr, ctx = i["hxr"], i["ctx"]
            h, x = hxr[:, :hd], hxr[:, hd:hd + xd]
            with conv_mode(mode):
                ops.conv2d_k3_multi(dict(x=hxr[:, :hd + xd], U=i["Uzr"], bias=i["bzr"], out=z,
                                         gate=dict(mode=1, ctx=ctx, h=h, out2=rh), **kw),
                                    dict(x=x, U=i["Uqx"], out=qx, **kw))
                hh = h.clone(memory_format=torch.contiguous_format)
                ops.conv2d_k3_multi(dict(x=hxr[:, hd + xd:], U=i["Uqh"], bias=i["bq"], out=hh,
                                         gate=dict(mode=2, ctx=ctx[:, 2 * hd:], h=hh, z=i["z"], add=i["qx"]), **kw))
            return z, rh, qx, hh

        def oracle(i, outs):
            d = torch.Tensor.double
            z, rh, qx, hh = (o[:1, ..., :W].cpu() for o in outs)
            hx, h, x = d(hxr[:, :hd + xd, :, :W]), d(hxr[:, :hd, :, :W]), d(hxr[:, hd:hd + xd, :, :W])
            c_ = d(ctx[..., :W])
            z_ref = torch.sigmoid(conv_ref(mode, hx, wz, bz) + c_[:, :hd])
            r_ref = torch.sigmoid(conv_ref(mode, hx, wr, br) + c_[:, hd:2 * hd])
            # test_wino4_gru_gate_epilogues' / test_mixed_gru_gate_epilogues' tolerances
            tol, tz = dict(atol=1e-4, rtol=1e-4), dict(atol=3e-5, rtol=1e-4)
            torch.testing.assert_close(z, z_ref.float(), **tz)
            torch.testing.assert_close(rh, (r_ref * h).float(), **tz)
            torch.testing.assert_close(qx, conv_ref(mode, x, wq[:, hd:].contiguous()).float(), **tol)
            q_ref = torch.tanh(conv_ref(mode, hxr[:, hd + xd:, :, :W], wq[:, :hd].contiguous(), bq)
                               + d(qx0[..., :W]) + c_[:, 2 * hd:])
            torch.testing.assert_close(hh, ((1 - d(z0[..., :W])) * h + d(z0[..., :W]) * q_ref).float(), **tol)
            if pitch:
                assert not any(bool(o[..., W:].any()) for o in outs)
        return inputs, call, oracle, dict(dests=dests)
    return build


for _mode in ("fp32", "split", "mixed"):
    case(f"conv2d_k3_multi[{_mode} gate epilogues 8x128]")(gate_case(_mode))
case("conv2d_k3_multi[split gate epilogues, pitched 8x124 of 128]")(gate_case("split", pitch=4))


def flow_head_case(mode):
    """flow_head_update (conv1 on F(4x4) with the channel-0 taps of conv2 summed in its epilogue, then the
    reduce): coords_x += delta in place (every call starts from a copy), flow planes refreshed."""
    def build():
        C, Cm, H, W = 32, 64, 9, 36
        h, cx = rnd(1, C, H, W, seed=1), rnd(1, 1, H, W, seed=2) * 5 + 10
        w1, b1 = rnd(Cm, C, 3, 3, seed=3) / (3 * C ** 0.5), rnd(Cm, seed=4) * 0.1
        w2, b2 = rnd(2, Cm, 3, 3, seed=5) / (3 * Cm ** 0.5), rnd(2, seed=6) * 0.1

        def inputs(rep):
            with conv_mode(mode):
                U1 = ops.wino_weights(w1.to(dev))
            return rep(h), rep(cx), U1, b1.to(dev), w2.to(dev), b2.to(dev)

        def dests(inp):
            return (torch.empty(inp[0].shape[0], 2, H, W, device=dev),)

        def call(inp, dests):
            hs, cxs, U1, b1g, w2g, b2g = inp
            cur = cxs.clone()
            with conv_mode(mode):
                assert ops.flow_head_update(hs, U1, b1g, w2g, b2g, cur, dests[0])
            return cur, dests[0]

        def oracle(inp, outs):
            d = torch.Tensor.double
            delta = F.conv2d(torch.relu(conv_ref(mode, h, w1, b1)), d(w2), d(b2), padding=1)[:, :1]
            tol = dict(atol=2e-5, rtol=1e-4)   # test_flow_head_fused_matches_separate's / test_mixed_flow_head's
            torch.testing.assert_close(outs[0][:1].cpu(), (d(cx) + delta).float(), **tol)
            x0 = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
            torch.testing.assert_close(outs[1][:1, :1].cpu(), outs[0][:1].cpu() - x0, atol=2e-5, rtol=1e-5)
            assert not outs[1][:, 1].any()
        return inputs, call, oracle, dict(dests=dests)
    return build


for _mode in ("fp32", "split", "mixed"):
    case(f"flow_head_update[{_mode} 32->64 9x36]")(flow_head_case(_mode))


def pitched_conv_case(mode):
    """conv2d_k3_multi on pitched planes (W 33 in a pitch of 36: columns 33 .. 35 zero, and zero after)."""
    def build():
        Cin, Cout, H, W, P = 16, 64, 9, 33, 36
        x = rnd(1, Cin, H, P, seed=21)
        x[..., W:] = 0.0
        w, b = rnd(Cout, Cin, 3, 3, seed=22) / (3 * Cin ** 0.5), rnd(Cout, seed=23)

        def inputs(rep):
            with conv_mode(mode):
                U = ops.wino_weights(w.to(dev))
            return rep(x), U, b.to(dev)

        def dests(inp):
            return (torch.empty(inp[0].shape[0], Cout, H, P, device=dev),)

        def call(inp, dests):
            dests[0][..., W:] = 0.0
            with conv_mode(mode):
                (res,) = ops.conv2d_k3_multi(dict(x=inp[0], U=inp[1], bias=inp[2], relu=True, out=dests[0], width=W))
            return (res,)

        def oracle(inp, outs):
            ref = torch.relu(F.conv2d(x[..., :W].double(), w.double(), b.double(), padding=1))
            got = outs[0][:1, ..., :W].cpu()
            if mode == "mixed":
                rel = float((got - ref.float()).abs().mean() / ref.abs().mean())
                assert 2e-4 < rel < 5e-3, rel
            else:
                torch.testing.assert_close(got, ref.float(), atol=1e-4, rtol=1e-4)   # test_wino4_pitched_planes'
            assert not outs[0][..., W:].any()
        return inputs, call, oracle, dict(dests=dests)
    return build


for _mode in ("fp32", "split", "mixed"):
    case(f"conv2d_k3_multi[{_mode} pitched 9x33 of 36]")(pitched_conv_case(_mode))


# -------------------------------------------------------------------------------------- other convs
@contextlib.contextmanager
def direct_split(on):
    saved, ops.DIRECT_SPLIT = ops.DIRECT_SPLIT, on
    try:
        yield
    finally:
        ops.DIRECT_SPLIT = saved


def conv_direct_case(form, split, guard=False):
    """tests/test_gpu_direct.py's three forms at its smaller shapes: the 7x7 stem, the stride-2 3x3 with
    its fused 1x1 downsample, and that conv with the residual block's close formed on load; statistics
    on (partials compared).  guard: a patch times 1e5 fires the split kernel's range guard (P4)."""
    def build():
        if form == "stem":
            Cin, Cout, H, W, K, S = 3, 64, 33, 29, 7, 1
            x, w, wd = rnd(1, Cin, H, W, seed=1), rnd(Cout, Cin, 7, 7, seed=2) / 10, None
        else:
            Cin, Cout, H, W, K, S = 64, 96, 27, 45, 3, 2
            x = rnd(1, Cin, H, W, seed=3) if form == "s2" else rnd(1, Cin, H, W, seed=6) * 3 + 0.5
            w, wd = rnd(Cout, Cin, 3, 3, seed=4) / (3 * Cin ** 0.5), rnd(Cout, Cin, 1, 1, seed=5) / Cin ** 0.5
        skip, mean, rstd = torch.relu(rnd(1, Cin, H, W, seed=7)), rnd(1, Cin, seed=8) * 0.3, rnd(1, Cin, seed=9).abs() + 0.2
        if guard:   # (past the f16 range, |x| >= 65520, as test_split_range_guard)
            x[0, :, 4:9, 10:20] *= 1e5

        def inputs(rep):
            with direct_split(split):
                wg_ = ops.conv_direct_weights(w.to(dev), S)
                wd_ = None if wd is None else ops.conv_direct_weights(wd.to(dev), S, with_ds=True)
            assert (wg_.dtype == torch.int32) == split
            return rep(x), wg_, wd_, rep(skip), rep(mean).reshape(-1), rep(rstd).reshape(-1)

        def call(inp, dests):
            xs, wg_, wd_, sk, m, r = inp
            B = xs.shape[0]
            with capture_partials() as parts:
                res = ops.conv_direct(xs, wg_, K, S, Cout, wd=wd_, stats=True, close=(sk, m, r) if form == "close" else None)
            outs, stats = res[:-1], res[-1]
            return tuple(outs) + tuple(p.view(B, -1) for p in parts) + tuple(t.view(B, -1) for st in stats for t in st)

        def oracle(inp, outs):
            xin = x
            if form == "close":
                xin = torch.relu(torch.relu((x - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)) + skip)
            ref = F.conv2d(xin.double(), w.double(), stride=S, padding=K // 2).float()
            got = outs[0][:1].cpu()
            if guard:   # test_split_range_guard's
                assert torch.isfinite(got).all() and float((got - ref).abs().max()) < 1e-5 * float(ref.abs().max())
                return
            torch.testing.assert_close(got, ref, atol=2e-5, rtol=1e-4)
            n = 1 if wd is None else 2
            if wd is not None:
                torch.testing.assert_close(outs[1][:1].cpu(), F.conv2d(xin.double(), wd.double(), stride=S).float(),
                                           atol=2e-5, rtol=1e-4)
            torch.testing.assert_close(outs[2 * n][0].cpu(), ref.mean(dim=(2, 3)).flatten(), atol=1e-5, rtol=1e-5)
            torch.testing.assert_close(outs[2 * n + 1][0].cpu(),
                                       1 / torch.sqrt(ref.var(dim=(2, 3), unbiased=False).flatten() + 1e-5),
                                       atol=1e-4, rtol=1e-4)

        def guard_fired(inp):
            assert redo_blocks() > 0, "the range guard did not fire"
        hooks = dict(before=lambda inp: redo_blocks(), after=guard_fired) if guard else {}
        return inputs, call, oracle, hooks
    return build


for _form in ("stem", "s2", "close"):
    for _split in (False, True):
        case(f"conv_direct[{_form} {'split' if _split else 'fp32'}]", streams=_split)(conv_direct_case(_form, _split))
case("conv_direct[stem split range guard]", streams=True)(conv_direct_case("stem", True, guard=True))
case("conv_direct[s2 split range guard]", streams=True)(conv_direct_case("s2", True, guard=True))


def small_conv_case(what, guard=False):
    """conv1x1 (split-f16 MFMA 1x1; guard: two rows times 1e5, past the f16 range, as test_conv1x1_range_guard,
    so those blocks run again on fp32 FMAs and the process-global redo counter moves), conv2d_small (convf1's 2 -> 64 7x7), conv2d_k3_narrow (-> 2 channels),
    norm_act (affine + ReLU + skip into a channel slice), plane_stats; their own tests' tolerances."""
    def build():
        if what == "conv1x1":
            Cin, Cout, H, W = 64, 96, 9, 36
            x, w, b = rnd(1, Cin, H, W, seed=1), rnd(Cout, Cin, 1, 1, seed=2) / Cin ** 0.5, rnd(Cout, seed=3)
        elif what == "conv2d_small":
            Cin, Cout, H, W = 2, 64, 37, 53
            x, w, b = rnd(1, Cin, H, W, seed=21), rnd(64, 2, 7, 7, seed=22) * 0.1, rnd(64, seed=23) * 0.1
        elif what == "narrow":
            Cin, Cout, H, W = 64, 2, 9, 13
            x, w, b = rnd(1, Cin, H, W, seed=31), rnd(2, Cin, 3, 3, seed=32) / (3 * Cin ** 0.5), rnd(2, seed=33)
        else:
            Cin, Cout, H, W = 64, 64, 9, 13
            x, w, b = rnd(1, Cin, H, W, seed=41) * 2 + 0.3, None, None
        skip, s, t = rnd(1, Cin, H, W, seed=42), rnd(Cin, seed=43).abs() + 0.5, rnd(Cin, seed=44)
        if guard:
            x[:, :, :2] *= 1e5

        def inputs(rep):
            g = lambda a: None if a is None else a.to(dev)   # noqa: E731
            wk = g(w)
            if what == "conv1x1":
                wk = ops.conv1x1_weights(g(w))
                assert wk is not None
            elif what == "conv2d_small":
                wk = g(w).permute(1, 2, 3, 0).contiguous()
            return rep(x), wk, g(b), rep(skip), g(s), g(t)

        def dests(inp):
            B = inp[0].shape[0]
            return (torch.empty(B, 2 * Cout, H, W, device=dev),) if what in ("conv1x1", "norm_act") else ()

        def call(inp, dests):
            xs, wk, bias, sk, sg, tg = inp
            B = xs.shape[0]
            if what == "conv1x1":
                return (ops.conv1x1(xs, wk, Cout, bias, 0.25, out=dests[0][:, Cout:]),)
            if what == "conv2d_small":
                return (ops.conv2d_small(xs, wk, bias, 64, 7, relu=True),)
            if what == "narrow":
                return (ops.conv2d_k3_narrow(xs, wk, bias),)
            if what == "norm_act":
                return (ops.norm_act(xs, ops.Affine(None, sg, tg), act_in="relu", skip=sk, act_out="relu",
                                     out=dests[0][:, Cout:]),)
            return tuple(v.view(B, -1) for v in ops.plane_stats(xs))

        def oracle(inp, outs):
            xd = x.double()
            got = outs[0][:1].cpu()
            if what == "conv1x1" and guard:   # test_conv1x1_range_guard's
                ref = 0.25 * F.conv2d(xd, w.double(), b.double())
                assert torch.isfinite(got).all()
                np.testing.assert_allclose(got.double().numpy(), ref.numpy(), rtol=1e-5, atol=2e-6 * float(ref.abs().max()))
            elif what == "conv1x1":   # test_conv1x1_matches_conv2d's: 2e-6 of max |y|
                ref = 0.25 * F.conv2d(xd, w.double(), b.double())
                assert float((got.double() - ref).abs().max()) < 2e-6 * float(ref.abs().max())
            elif what == "conv2d_small":
                torch.testing.assert_close(got, torch.relu(F.conv2d(xd, w.double(), b.double(), padding=3)).float(),
                                           atol=2e-5, rtol=1e-5)
            elif what == "narrow":
                torch.testing.assert_close(got, F.conv2d(xd, w.double(), b.double(), padding=1).float(), atol=2e-5, rtol=1e-5)
            elif what == "norm_act":
                ref = torch.relu(torch.relu(xd * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1)) + skip.double())
                torch.testing.assert_close(got, ref.float(), atol=1e-5, rtol=1e-5)
            else:
                torch.testing.assert_close(got[0], xd.mean(dim=(2, 3)).flatten().float(), atol=1e-5, rtol=1e-5)
                torch.testing.assert_close(outs[1][0].cpu(), (xd.var(dim=(2, 3), unbiased=False) + 1e-5).rsqrt().flatten().float(),
                                           atol=1e-4, rtol=1e-4)

        def redo():
            return int(N.lib().sa_conv1x1_redo_blocks(1))

        def guard_state(inp):   # around the first poisoned launch (the counter is read and reset)
            n = redo()
            assert n > 0 if guard else n == 0, f"conv1x1 redid {n} blocks"
        hooks = dict(before=lambda inp: redo(), after=guard_state) if what == "conv1x1" else {}
        return inputs, call, oracle, dict(dests=dests, **hooks)
    return build


for _what in ("conv1x1", "conv2d_small", "narrow", "norm_act", "plane_stats"):
    # conv1x1 is a guarded kernel with a process-global redo counter: P4, here and with the guard fired
    case({"narrow": "conv2d_k3_narrow"}.get(_what, _what), streams=_what == "conv1x1")(small_conv_case(_what))
case("conv1x1[range guard]", streams=True)(small_conv_case("conv1x1", guard=True))


# ------------------------------------------------------------------------- more regression and glue
def mask_upsample_case(guard=False):
    """tests/test_gpu_mask_upsample.py's case at 7 x 13 (ragged tiles, more than one 48-pixel block), Cin 256.
    guard: one input element at 7e4, past the f16 range, as test_mask_upsample_range_guard: its block
    computes its logits with fp32 FMAs and the process-global redo counter moves (P4 on both)."""
    def build():
        def inputs(rep):
            import test_gpu_mask_upsample as mu
            x, w, b, flow = mu._case(1, 256, 7, 13, 713)
            if guard:
                x[0, 37, 4, 9] = 7e4
            ws = ops.conv1x1_weights(w)
            assert ws is not None
            return dict(x=rep(x), flow=rep(flow), ws=ws, b=b, one=(x, w, b, flow))

        def call(i, dests):
            return (ops.mask_upsample(i["x"], i["ws"], i["b"], 0.25, i["flow"]),)

        def oracle(i, outs):
            import test_gpu_mask_upsample as mu
            x, w, b, flow = i["one"]
            # (the two kernels' guarded blocks cover different pixels: bit-equal to the unfused pair without the guard only)
            mu._check(outs[0][:1], x, w, b, 0.25, flow, i["ws"], "mask_upsample 7x13", bit_equal=not guard)

        def redo():
            return int(N.lib().sa_mask_upsample_redo_blocks(1))

        def guard_state(i):   # around the first poisoned launch (the counter is read and reset)
            n = redo()
            assert n > 0 if guard else n == 0, f"mask_upsample redid {n} blocks"
        return inputs, call, oracle, dict(before=lambda i: redo(), after=guard_state)
    return build


case("mask_upsample[256 7x13]", streams=True)(mask_upsample_case())
case("mask_upsample[256 7x13 range guard]", streams=True)(mask_upsample_case(guard=True))


def mirror_case():
    """mono_scale_mirror of test_mirror_and_coords (one sample; scale and shift are per sample)."""
    def build():
        rng = np.random.default_rng(2)
        H, W = 8, 40
        mde, conf = (rng.random((1, 2, H, W)).astype(f32) for _ in range(2))
        disp = (rng.random((1, 2, H, W)) * 20).astype(f32)
        scale, shift = np.array([[12.0]], f32), np.array([[1.5]], f32)

        def inputs(rep):
            return rep(mde), rep(scale).reshape(-1), rep(shift).reshape(-1), rep(disp), rep(conf)

        def call(inp, dests):
            return tuple(ops.mono_scale_mirror(*inp, 1.0, 0.98))

        def oracle(inp, outs):
            rsm2 = (scale[0, 0] * mde[:, 0:1] + shift[0, 0]).astype(f32)
            rsm3 = (scale[0, 0] * mde[:, 1:2] + shift[0, 0]).astype(f32)
            close(outs[0][:1], rsm2, atol=1e-5)
            close(outs[1][:1], rsm3, atol=1e-5)
            lrc, _ = R.softlrc(rsm2, rsm3, 1.0)
            close(outs[2][:1], R.handcrafted_mirror_detector(disp[:, 0:1], rsm2, conf[:, 0:1], lrc, 0.98), atol=2e-5)
            close(outs[3][:1], np.arange(W, dtype=f32) - rsm2, atol=1e-5)
        return inputs, call, oracle
    return build


case("mono_scale_mirror[8x40]")(mirror_case())


def flow_update_case(H, W):
    """flow_update: coords_x += delta in place (every call starts from a copy); both flow planes refreshed."""
    def build():
        cx, delta = rnd(1, 1, H, W, seed=H) * 4 + 8, rnd(1, 2, H, W, seed=W)

        def inputs(rep):
            return rep(cx), rep(delta)

        def dests(inp):
            B = inp[0].shape[0]
            return torch.empty(B, 2, H, W, device=dev), torch.empty(B, 2, H, W, device=dev)

        def call(inp, dests):
            cur = inp[0].clone()
            ops.flow_update(cur, inp[1], dests[0], dests[1])
            return (cur,) + tuple(dests)

        def oracle(inp, outs):
            want = cx + delta[:, :1]
            torch.testing.assert_close(outs[0][:1].cpu(), want, atol=1e-6, rtol=0)
            x0 = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
            for fl in outs[1:]:
                torch.testing.assert_close(fl[:1, :1].cpu(), want - x0, atol=1e-5, rtol=0)
                assert not fl[:, 1].any()
        return inputs, call, oracle, dict(dests=dests)
    return build


case("flow_update[9x13]")(flow_update_case(9, 13))
case("flow_update[10x12]")(flow_update_case(10, 12))


# ------------------------------------------------------------------------------------------- tiler
def tiler_case(what):
    """The ragged geometry of test_tile_gather_and_stitch_equal_torch_path (200 x 260 in 96 x 128 tiles,
    overlap 32).  The tiler works on one image, so the replicas are along the tile axis: every origin
    (every tile, for the stitch) is listed R times, and each copy must give the same padded tile;
    the stitch adds R copies of every tile into one image (num, den: in-place sums from zero)."""
    def build():
        from stereoanywhere_amd import tiler
        H, W, th, tw, ov = 200, 260, 96, 128, 32
        src = torch.rand(1, 3, H, W, generator=torch.Generator(device="cpu").manual_seed(H + W))
        tiles = list(dict.fromkeys(tiler.enumerate_tiles(H, W, th, tw, ov)))
        org = [(s.y_start, s.x_start) for s in tiles]
        pad = tiler.pad32(th, tw)
        R_ = 8

        def inputs(rep):
            if what == "gather":
                return (src.to(dev),)
            disp = torch.rand(len(tiles), 1, th, tw, generator=torch.Generator(device="cpu").manual_seed(5)).to(dev)
            return disp, tiler.blend_weight(th, tw, dev).contiguous()

        def dests(inp):
            return () if what == "gather" else tuple(torch.empty(H, W, device=dev) for _ in range(4))

        def call(inp, dests):
            if what == "gather":   # [R * n, ...] with copy r of tile t at r * n + t -> [R, n, ...]
                out = ops.tile_gather_pad(inp[0], org * R_, th, tw, pad)
                return (out.view(R_, len(org), *out.shape[1:]),)
            listed = [(y, x, k) for _ in range(R_) for k, (y, x) in enumerate(org)]
            for t in dests:
                t.zero_()
            ops.tile_stitch(inp[0], listed, inp[1], H, W, True, dests[0], dests[1])    # the quotient in num
            ops.tile_stitch(inp[0], listed, inp[1], H, W, False, dests[2], dests[3])   # the two sums
            return dests[0][None], dests[2][None], dests[3][None]   # (one image: no replica axis, no P1)

        def oracle(inp, outs):
            if what == "gather":
                want = F.pad(torch.cat([src[:, :, y:y + th, x:x + tw] for y, x in org]), pad, mode="replicate")
                assert torch.equal(outs[0][0].cpu(), want)
                return
            st, wt = torch.zeros(H, W, device=dev), torch.zeros(H, W, device=dev)
            for y, x, k in [(y, x, k) for _ in range(R_) for k, (y, x) in enumerate(org)]:   # the torch loop
                st[y:y + th, x:x + tw] += inp[0][k, 0] * inp[1]
                wt[y:y + th, x:x + tw] += inp[1]
            want = torch.where(wt > 0, st / torch.clamp(wt, min=1e-4), st)
            assert torch.equal(outs[0][0], want) and torch.equal(outs[1][0], st) and torch.equal(outs[2][0], wt)
        return inputs, call, oracle, dict(dests=dests)
    return build


case("tile_gather_pad[200x260]")(tiler_case("gather"))
case("tile_stitch[200x260]", p1=False)(tiler_case("stitch"))


# ---------------------------------------------------------------------------- the other backward ops
def corr_backward_case(what):
    """corr_lookup_backward, pyramid_backward, corr_volume_backward at H 3, W1 37, W2 45 (ragged), against
    float64 restatements of the adjoints; fp32 sums of at most 256 terms: 2e-6 of max |ref| as the forward's."""
    def build():
        C, H, W1, W2, L, r = 64, 3, 37, 45, 4, 4
        rng = np.random.default_rng(W1 + W2)
        f2, f3 = fmaps(C, H, W1, W2)
        gv = rng.standard_normal((1, H, W1, W2)).astype(f32)
        go = rng.standard_normal((1, L * (2 * r + 1), H, W1)).astype(f32)
        cx = (rng.random((1, 1, H, W1)) * (W2 + 40) - 20).astype(f32)

        def inputs(rep):
            if what == "lookup":
                return rep(go), rep(cx)
            if what == "pyramid":
                B = rep(cx).shape[0]
                return (ops.corr_lookup_backward(rep(go), rep(cx), W2, L, r),)   # a pyramid-shaped gradient
            return rep(gv), rep(f2), rep(f3)

        def call(inp, dests):
            B = inp[0].shape[0] if what != "pyramid" else inp[0].shape[0] // (H * W1)
            if what == "lookup":
                return (by_sample(ops.corr_lookup_backward(*inp, W2, L, r), B),)
            if what == "pyramid":
                return (by_sample(ops.pyramid_backward(inp[0], W2, L), B),)
            return tuple(ops.corr_volume_backward(*inp))

        def oracle(inp, outs):
            if what == "volume":
                g2 = np.einsum("bhjk,bchk->bchj", gv.astype(np.float64), f3.astype(np.float64)) / np.sqrt(np.float64(C))
                g3 = np.einsum("bhjk,bchj->bchk", gv.astype(np.float64), f2.astype(np.float64)) / np.sqrt(np.float64(C))
                close(outs[0][:1], g2, atol=2e-6 * np.abs(g2).max() + 1e-6)
                close(outs[1][:1], g3, atol=2e-6 * np.abs(g3).max() + 1e-6)
                return
            rs, offs, wids = ops.pyramid_geometry(W2, L)
            if what == "pyramid":   # grad_volume[k] = sum_l 2^-l grad_level_l[k >> l]
                gp = c(inp[0])[:H * W1].astype(np.float64)
                k = np.arange(W2)
                want = sum(2.0 ** -l * gp[:, offs[l] + np.minimum(k >> l, wids[l] - 1)] * ((k >> l) < wids[l]) for l in range(L))
                close(outs[0][0], want, atol=1e-6 * max(1.0, np.abs(want).max()))
                return
            # the adjoint identity against the forward lookup: <lookup(p), g> = <p, lookup_backward(g)>
            p = np.zeros((H * W1, rs), f32)
            for o, w_ in zip(offs, wids):
                p[:, o:o + w_] = rng.standard_normal((H * W1, w_))
            pg = torch.from_numpy(p).to(dev)
            fwd = ops.corr_lookup(pg, None, W2, L, r, inp[1][:1].contiguous()).double()
            lhs = float((fwd * torch.from_numpy(go).to(dev).double()).sum())
            rhs = float((pg.double() * outs[0][0].double()).sum())
            assert abs(lhs - rhs) <= 1e-5 * float((fwd.abs() * torch.from_numpy(np.abs(go)).to(dev).double()).sum())
            assert not outs[0][0][:, offs[-1] + wids[-1]:].any()   # the row padding is written, zero
        return inputs, call, oracle
    return build


case("corr_lookup_backward[3x37x45]")(corr_backward_case("lookup"))
case("pyramid_backward[3x37x45]")(corr_backward_case("pyramid"))
case("corr_volume_backward[64x3x37x45]")(corr_backward_case("volume"))


def diffops_backward_case(what):
    """softargmin_conf_backward (reference layout, n 64: the strided side's workspace is a torch.empty)
    and convex_upsample_backward (7 x 13), with test_gpu_diffops_backward.py's yardstick: against
    torch.autograd in float64, within 4 x the error of the same autograd in float32."""
    def build():
        import diffops_ref as dref
        rng = np.random.default_rng(64)
        if what == "softargmin":
            H, n = 3, 64
            vols = (rng.standard_normal((1, 2, H, n, n)) * 4).astype(f32)
            gs = [rng.standard_normal((1, H, n)).astype(f32) for _ in range(4)]
        else:
            H, W = 7, 13
            flow = (rng.standard_normal((1, 1, H, W)) * 5).astype(f32)
            mask = (rng.standard_normal((1, 144, H, W)) * 3).astype(f32)
            gout = rng.standard_normal((1, 1, 4 * H, 4 * W)).astype(f32)

        def inputs(rep):
            if what == "softargmin":
                return (rep(vols),) + tuple(rep(g) for g in gs)
            return rep(flow), rep(mask), rep(gout)

        def call(inp, dests):
            if what == "softargmin":
                t = inp[0]
                return tuple(ops.softargmin_conf_backward(t[:, 0], t[:, 1], (2 * H * n * n, n * n, n, 1),
                                                          (t.shape[0], H, n, n), *inp[1:]))
            return tuple(ops.convex_upsample_backward(*inp, 4))

        def oracle(inp, outs):
            if what == "softargmin":
                w64 = dref.softargmin_grads(vols[:, 0], vols[:, 1], gs, torch.float64)
                w32 = dref.softargmin_grads(vols[:, 0], vols[:, 1], gs, torch.float32)
            else:
                w64 = dref.convex_grads(flow, mask, gout, 4, True, torch.float64)
                w32 = dref.convex_grads(flow, mask, gout, 4, True, torch.float32)
            for a, x64, x32 in zip(outs, w64, w32):
                got = c(a)[:1].astype(np.float64)
                assert np.isfinite(got).all() and np.abs(got - x64).max() <= 4 * np.abs(x32 - x64).max()
        return inputs, call, oracle
    return build


case("softargmin_conf_backward[reference 64]")(diffops_backward_case("softargmin"))
case("convex_upsample_backward[7x13]")(diffops_backward_case("convex"))


def loss_case():
    """loss_terms and loss_terms_backward on tests/test_gpu_losses.py's problem (B 2, 9 x 33, every term):
    the outputs are sums over the whole batch and gradients scaled by batch-wide counts, so there is no
    replica to compare (no P1); reruns, dirty memory (the fp64 workspace and record are torch.empty) and
    the oracle stay."""
    def build():
        def inputs(rep):
            import test_gpu_losses as tl
            maps, kw = tl.problem(9, 33, "all")
            g = tl.g
            return dict(maps=maps, hm=tl.hip_maps(maps), up=torch.tensor([tl.UP], device=dev),
                        args=(g(kw["gt"]), g(kw["valid"]), kw["maxdisp"], g(kw["target"]), kw["gain"], kw["border"], kw["lrc_th"]))

        def run(i):
            out, rec = ops.loss_terms(i["hm"], *i["args"])
            gm, gc = ops.loss_terms_backward(i["hm"], *i["args"], rec, i["up"], None, [M.conf is not None for M in i["maps"]])
            return out, rec, gm, gc

        def call(i, dests):
            out, rec, gm, gc = run(i)
            return (out[None], rec[None]) + tuple(t for t in gm + gc if t is not None)

        def oracle(i, outs):
            import test_gpu_losses as tl
            hip = run(i)
            tl.check_all("loss_terms 9x33", i["maps"], hip, hip, *tl.reference(9, 33, "all"))
        return inputs, call, oracle
    return build


case("loss_terms + loss_terms_backward[9x33]", p1=False)(loss_case())


# ------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_invariance(case):
    got = run_case(case)
    print(case.name, got)


# ------------------------------------------------------------------------------- the harness itself
def test_poison_self_check_fails_when_the_poison_did_not_take():
    """The self-check is not vacuous: after poisoning with one word, a probe for the other word fails
    as "poison did not take"; the right word passes, for a small-pool and a large-pool size."""
    for nbytes in (68, 6 << 10, 3 << 20):
        poison_free_memory(torch.device(dev), 1 << 20, nbytes, -1)
        check_poison(torch.device(dev), nbytes, -1)
        with pytest.raises(PoisonDidNotTake, match="poison did not take"):
            check_poison(torch.device(dev), nbytes, 0)


def test_a_case_that_reads_before_it_writes_fails():
    """A 'kernel' that accumulates into its torch.empty output is caught by P3, and one whose result
    depends on the batch position by P1: the harness fails the cases it is there to fail."""
    def inputs(rep):
        return (rep(torch.arange(300.0).view(1, 300)),)

    def dirty(inp, dests):
        out = torch.empty_like(inp[0])
        out += inp[0]
        return (out,)

    def by_position(inp, dests):
        out = inp[0].clone()
        out[3, 7] += 1.0
        return (out,)
    with pytest.raises(AssertionError, match="P3"):
        run_case(Case("dirty", inputs, dirty, lambda inp, outs: None))
    with pytest.raises(AssertionError, match="P1"):
        run_case(Case("by_position", inputs, by_position, lambda inp, outs: None))

"""The differentiable HIP drop-ins at their sites in the reference's training forward and backward
(tests/golden/make_golden_insitu.py: the reference's own autograd, captured once on the CPU), site by site and as the
volume head of stereoanywhere.py:174-271 composed the way INTEGRATION.md section 2 says.

Per site: the drop-in runs under autograd on the captured inputs; its forward is held to the captured output at the
tolerance of the op's own forward test against the reference's vectors (tests/test_gpu_ops.py's constants, as
imported), its backward runs from the captured output gradients, and every input gradient is held to the float64 restatement's, which tests/test_insitu_ref_cpu.py pins to
the capture: max |hip - r64| <= 4 e_ref with e_ref = max |captured - r64|, the reference's own float32 error (the
suite's standing criterion; none of these ops' own autograd tests adds a floor), or the op's derived bound where it
has one.  err / e_ref is printed for every tensor."""
import copy

import numpy as np
import pytest
import torch

import insitu_util as I
import test_gpu_ops as T
import volume_stage_ref
from stereoanywhere_amd import diffops
from stereoanywhere_amd.corr import HipCorrBlock1D
from test_gpu_corr_backward import extract_A
from test_gpu_hourglass_convs import convs_taken  # noqa: F401 (a fixture)
from test_gpu_upcat_conv_autograd import joins_taken  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
dev = "cuda"
U = I.U


@pytest.fixture(scope="module")
def cap():
    fix, meta = I.load()
    c = dict(fix)
    for s in I.S3_RUNS:
        c.update(I.s3_captured_sums(fix, s))
    c["s4.fused.g_d2"], c["s4.fused.g_d3"] = fix["s4.lrc0.g_d2"], fix["s4.lrc0.g_d3"]
    c.update(I.head_captured(fix))
    return c, meta


def g(a, grad=False):
    x = I.t(a, device=dev)
    return x.requires_grad_() if grad else x


def forward(name, got, captured, tol):
    err = float(np.abs(I.n64(got) - captured).max())
    print(f"{name}: forward max |hip - captured| {err:.3g}, {err / tol:.3g} of the tolerance {tol:.3g}")
    assert tuple(got.shape) == captured.shape, name
    assert err <= tol, name


def backward(name, got, c, r64, key=None):
    key = key or name
    assert got is not None, f"{name}: no gradient"
    e_ref = I.e_ref(c, r64, key)
    err = float(np.abs(I.n64(got) - r64[key]).max())
    print(f"{name}: err {err:.3g}, e_ref {e_ref:.3g} ({e_ref / np.abs(r64[key]).max():.2g} of max |g|), "
          f"err / e_ref {err / e_ref:.3g}")
    assert tuple(got.shape) == r64[key].shape, name
    assert err <= 4 * e_ref, name


# ----------------------------------------------------------------------------------- S1
def test_s1_corr_volume(cap):
    """HipCorrBlock1D.corr at :135.  The gradients: (K + 3) u sum |terms| of
    tests/test_gpu_corr_backward.py::test_corr_volume_backward, K = W2 / W1."""
    c, _ = cap
    r64, mag = I.site_s1(c)
    f2, f3 = g(c["s1.f2"], True), g(c["s1.f3"], True)
    vol = HipCorrBlock1D.corr(f2, f3)
    assert vol.grad_fn is not None
    forward("s1.out", vol, c["s1.out"], T.TOL_CORR_VOLUME)
    vol.backward(g(c["s1.g_out"]))
    for k, t, K in (("s1.g_f2", f2, f3.shape[3]), ("s1.g_f3", f3, f2.shape[3])):
        err, bound = np.abs(I.n64(t.grad) - r64[k]), (K + 3) * U * mag[k]
        e_ref = I.e_ref(c, r64, k)
        print(f"{k}: err {err.max():.3g}, largest fraction of the bound {(err[bound > 0] / bound[bound > 0]).max():.3g}, "
              f"e_ref {e_ref:.3g}, err / e_ref {err.max() / e_ref:.3g}")
        assert np.all(err <= bound), k


# ----------------------------------------------------------------------------------- S2
ROUTES = {"torch": {}, "closes": dict(closes="hip"), "closes+joins": dict(closes="hip", joins="hip"),
          "closes+joins+convs": dict(closes="hip", joins="hip", convs="hip")}


@pytest.fixture(scope="module")
def hourglass(cap):
    c, meta = cap
    hg = I.hourglass_module(meta)
    return hg, I.run_hourglass(c, copy.deepcopy(hg), torch.float64)


@pytest.mark.parametrize("route", list(ROUTES))
def test_s2_hourglass(cap, hourglass, route, joins_taken, convs_taken):  # noqa: F811
    """blocks.Hourglass at :162 on the captured masked volume and feature maps, from the captured gradient of its
    output: the output, the gradients of the volume and of the feature maps, every parameter's gradient."""
    c, meta = cap
    hg, r64 = hourglass
    got = I.run_hourglass(c, copy.deepcopy(hg), torch.float32, dev, **ROUTES[route])
    assert joins_taken == ([True, False] if "joins" in route else [])
    assert convs_taken == ([(16, True), (32, True), (16, True), (16, True), (8, True), (8, True)] if "convs" in route else [])
    for k in sorted(r64):
        if r64[k] is None:
            assert got[k] is None, f"{k} is dead and must have no gradient"
            continue
        e_ref, err = I.e_ref(c, r64, k), float(np.abs(got[k] - r64[k]).max())
        print(f"{route} {k}: err {err:.3g}, e_ref {e_ref:.3g} ({e_ref / np.abs(r64[k]).max():.2g} of max), err / e_ref {err / e_ref:.3g}")
        assert err <= 4 * e_ref, (route, k)


# ----------------------------------------------------------------------------------- S3
@pytest.mark.parametrize("s", I.S3_RUNS)
def test_s3_softargmin(cap, s):
    """The four estimate_* calls at :174-177, and one softargmin_conf call in their place: the same maps, the same
    gradients at the volumes up to the order of autograd's sum.  s3: the run proper; s3p: the run with the
    classifiers' weights multiplied by 64 (one sharp peak on most lines, confidences up to 1)."""
    c, _ = cap
    r64 = I.site_s3(c, s=s)
    vd, vc = g(c[f"{s}.dL.vol"], True), g(c[f"{s}.cL.vol"], True)
    outs = (diffops.estimate_left_disparity(vd), diffops.estimate_right_disparity(vd),
            diffops.estimate_left_confidence(vc), diffops.estimate_right_confidence(vc))
    gouts = [g(c[f"{s}.{k}.g_out"]) for k, _ in I.S3]
    for (k, _), o in zip(I.S3, outs):
        forward(f"{s}.{k}.out", o, c[f"{s}.{k}.out"], T.TOL_SOFTARGMIN_DISP if k[0] == "d" else T.TOL_SOFTARGMIN_CONF)
    torch.autograd.backward(outs, gouts)
    backward(f"{s}.g_vol_disp", vd.grad, c, r64)
    backward(f"{s}.g_vol_conf", vc.grad, c, r64)
    jd, jc = g(c[f"{s}.dL.vol"], True), g(c[f"{s}.cL.vol"], True)
    joint = diffops.softargmin_conf(jd, jc)
    for o, j in zip(outs, joint):
        assert torch.equal(o, j)
    torch.autograd.backward(joint, gouts)
    backward(f"{s}.g_vol_disp (softargmin_conf)", jd.grad, c, r64, f"{s}.g_vol_disp")
    backward(f"{s}.g_vol_conf (softargmin_conf)", jc.grad, c, r64, f"{s}.g_vol_conf")


# ----------------------------------------------------------------------------------- S4
def test_s4_softlrc(cap):
    """softlrc at :186 and :199, and the products of :188-189: as softlrc followed by torch's product, and as one
    softlrc_conf call."""
    c, meta = cap
    th = meta["lrc_th"]
    r64 = I.site_s4(c, meta)
    d2, d3 = g(c["s4.lrc0.d2"], True), g(c["s4.lrc0.d3"], True)
    s2, s3 = diffops.softlrc(d2, d3, lrc_th=th)
    forward("s4.lrc0.s2", s2, c["s4.lrc0.s2"], T.TOL_SOFTLRC)
    forward("s4.lrc0.s3", s3, c["s4.lrc0.s3"], T.TOL_SOFTLRC)
    torch.autograd.backward([s2, s3], [g(c["s4.lrc0.g_s2"]), g(c["s4.lrc0.g_s3"])])
    backward("s4.lrc0.g_d2", d2.grad, c, r64)
    backward("s4.lrc0.g_d3", d3.grad, c, r64)
    q2, q3 = diffops.softlrc(g(c["s4.lrc1.d2"]), g(c["s4.lrc1.d3"]), lrc_th=th)
    forward("s4.lrc1.s2", q2, c["s4.lrc1.s2"], T.TOL_SOFTLRC)
    forward("s4.lrc1.s3", q3, c["s4.lrc1.s3"], T.TOL_SOFTLRC)
    results = {}
    for how in ("softlrc, product", "softlrc_conf"):
        d2, d3, c2, c3 = (g(c[k], True) for k in ("s4.lrc0.d2", "s4.lrc0.d3", "s4.and0.x", "s4.and1.x"))
        if how == "softlrc_conf":
            p2, p3 = diffops.softlrc_conf(d2, d3, c2, c3, lrc_th=th)
        else:
            s2, s3 = diffops.softlrc(d2, d3, lrc_th=th)
            p2, p3 = c2 * s2, c3 * s3
        forward(f"s4.and0.out ({how})", p2, c["s4.and0.out"], T.TOL_SOFTLRC)
        forward(f"s4.and1.out ({how})", p3, c["s4.and1.out"], T.TOL_SOFTLRC)
        torch.autograd.backward([p2, p3], [g(c["s4.and0.g_out"]), g(c["s4.and1.g_out"])])
        for key, x in (("s4.fused.g_d2", d2), ("s4.fused.g_d3", d3), ("s4.and0.g_x", c2), ("s4.and1.g_x", c3)):
            backward(f"{key} ({how})", x.grad, c, r64, key)
        results[how] = [p2, p3]
    # the fused product is the separate one: one fp32 multiplication of the same two values
    for a, b in zip(*results.values()):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------- S5
def test_s5_weighted_lsq(cap):
    c, _ = cap
    r64 = I.site_s5(c)
    m, d, cf = (g(c[f"s5.{k}"], True) for k in ("mde", "disp", "conf"))
    scale, shift = diffops.weighted_lsq(m, d, cf)
    for name, got, tol in (("s5.scale", scale, T.TOL_LSQ_SCALE), ("s5.shift", shift, T.TOL_LSQ_SHIFT)):
        print(f"{name}: forward max |hip - captured| {float(np.abs(I.n64(got) - c[name]).max()):.3g}")
        np.testing.assert_allclose(I.n64(got), c[name], **tol)
    torch.autograd.backward([scale, shift], [g(c["s5.g_scale"]), g(c["s5.g_shift"])])
    for k, x in (("s5.g_mde", m), ("s5.g_disp", d), ("s5.g_conf", cf)):
        backward(k, x.grad, c, r64)


# ----------------------------------------------------------------------------------- S6
def test_s6_truncation(cap):
    """truncate_volume, and volume_stage(plan=None, truncate=...), in place of :203 and the product at :254."""
    c, meta = cap
    r64 = I.site_s6(c, meta)
    atten = meta["mirror_attenuation"]
    vol = g(I.volume5(c["s1.out"]), True)
    disp, conf = g(c["s6.disp"], True), g(c["s6.conf"], True)
    prod = diffops.truncate_volume(vol, disp, conf, atten)
    want = torch.from_numpy(np.moveaxis(r64["s7.0.fullcorr"], 3, 1))
    volume_stage_ref.assert_close(prod, want, "s6 product (truncate_volume)")
    forward("s6 product against the capture", prod, I.volume5(c["s7.0.fullcorr"]),
            float(volume_stage_ref.tolerance(want).max()) + volume_stage_ref.E * float(want.abs().max()))
    prod.backward(g(I.volume5(c["s7.0.g_fullcorr"])))
    assert disp.grad is None and conf.grad is None
    backward("s1.g_out", vol.grad.squeeze(1).unsqueeze(3), c, r64)
    vol2, mono = g(I.volume5(c["s1.out"]), True), g(c["s3.dL.vol"], True)
    staged, mono_out = diffops.volume_stage(vol2, mono, None, None, truncate=(disp.detach(), conf.detach(), atten))
    assert mono_out is mono and torch.equal(staged, prod)
    staged.backward(g(I.volume5(c["s7.0.g_fullcorr"])))
    assert torch.equal(vol2.grad, vol.grad)


# ----------------------------------------------------------------------------------- S7
@pytest.mark.parametrize("b", [0, 1], ids=["stereo", "mono"])
def test_s7_lookups(cap, b):
    """Every iteration's lookup replayed on one HipCorrBlock1D per volume: the taps per iteration, and the summed
    gradient at fullcorr against (a) the float64 restatement with the kernel's own fp32 coefficients (extracted as
    tests/test_gpu_corr_backward.py does), within (5 iters + L + 8) u sum |terms|: the scatter's n + 1 <= 5 roundings
    per iteration and the sum over iterations, the fold's L - 1, second order; (b) the float64 restatement from the
    float64 coordinates, which the capture is pinned to, within 4 e_ref."""
    import corr_autograd_ref as ref
    c, meta = cap
    L, R, iters = meta["corr_levels"], meta["corr_radius"], meta["iters"]
    r64, _ = I.site_s7(c, meta)
    full = g(c[f"s7.{b}.fullcorr"], True)
    W2 = full.shape[-1]
    blk = HipCorrBlock1D(full, num_levels=L, radius=R)
    coords = [g(c[f"s7.{b}.{n}.coords"]) for n in range(iters)]
    taps = [blk(x) for x in coords]
    for n, tp in enumerate(taps):
        k = f"s7.{b}.{n}.taps"
        forward(k, tp, c[k], T.TOL_LOOKUP)
    torch.autograd.backward(taps, [g(c[f"s7.{b}.{n}.g_taps"]) for n in range(iters)])
    k = f"s7.{b}.g_fullcorr"
    backward(k, full.grad, c, r64)
    gp = agp = 0.0
    for n, x in enumerate(coords):
        A = extract_A(x[:, :1].contiguous(), W2, L, R)
        gp = gp + ref.lookup_backward(A, c[f"s7.{b}.{n}.g_taps"])
        agp = agp + ref.lookup_backward(A, np.abs(c[f"s7.{b}.{n}.g_taps"]))
    want = ref.pyramid_backward(gp, W2, L).reshape(full.shape)
    bound = (5 * iters + L + 8) * U * ref.pyramid_backward(agp, W2, L).reshape(full.shape)
    err = np.abs(I.n64(full.grad) - want)
    print(f"{k}: against the kernel's own coefficients: err {err.max():.3g}, largest fraction of the bound "
          f"{(err[bound > 0] / bound[bound > 0]).max():.3g}")
    assert np.all(err <= bound)


# ----------------------------------------------------------------------------------- S8
def test_s8_convex_upflow(cap):
    c, meta = cap
    r64 = I.site_s8(c, meta)
    for n in range(meta["iters"]):
        flow, mask = g(c[f"s8.{n}.flow"], True), g(c[f"s8.{n}.mask"], True)
        up = diffops.convex_upflow(flow, mask, n_downsample=meta["n_downsample"], use_scale_factor=True)
        forward(f"s8.{n}.up", up, c[f"s8.{n}.up"], T.TOL_CONVEX_UP)
        up.backward(g(c[f"s8.{n}.g_up"]))
        backward(f"s8.{n}.g_flow", flow.grad, c, r64)
        backward(f"s8.{n}.g_mask", mask.grad, c, r64)


# ----------------------------------------------------------------------------------- the composed head
class HipOps:
    """The drop-ins as INTEGRATION.md section 2 imports them."""
    softargmin_conf = staticmethod(diffops.softargmin_conf)
    softlrc_conf = staticmethod(diffops.softlrc_conf)
    weighted_lsq = staticmethod(diffops.weighted_lsq)
    corr_block = HipCorrBlock1D

    @staticmethod
    def softlrc(d2, d3, lrc_th):
        return diffops.softlrc(d2, d3, lrc_th=lrc_th)

    @staticmethod
    def volume_stage(stereo, mono, truncate):
        return diffops.volume_stage(stereo, mono, None, None, truncate=truncate)


def test_head(cap):
    """stereoanywhere.py:174-271 from the drop-ins and the torch glue between them (insitu_util.head: the
    interpolations, the sums at :194-197, the detached mirror detector), on the captured classifier volumes, stereo
    volume, mono maps and per-iteration detached coordinates; backward from the captured gradients of the six
    returned coarse entries and of every iteration's taps of both blocks.  The total gradients at the three input
    volumes against the float64 head, which the CPU test pins to the capture: a wrong detach, a missing consumer in
    the sum or a layout slip between two ops moves them by a fraction of their magnitude."""
    c, meta = cap
    o64, g64 = I.run_head(I.RefOps(torch.float64), c, meta, torch.float64)
    out, grads = I.run_head(HipOps, c, meta, torch.float32, dev)
    nd = 2 ** meta["n_downsample"]
    scale, shift = np.abs(c["s5.scale"]).max(), np.abs(c["s5.shift"]).max()
    mde_tol = nd * ((T.TOL_LSQ_SCALE["rtol"] * scale + T.TOL_LSQ_SCALE["atol"]) + T.TOL_LSQ_SHIFT["rtol"] * shift
                    + T.TOL_LSQ_SHIFT["atol"])   # (scale mde + shift) nd with mde <= 1
    for k, tol in (("dispmono2", nd * T.TOL_SOFTARGMIN_DISP), ("dispmono3", nd * T.TOL_SOFTARGMIN_DISP),
                   ("ldispmonoconf2", T.TOL_SOFTARGMIN_CONF), ("ldispmonoconf3", T.TOL_SOFTARGMIN_CONF),
                   ("scaled_mde2", mde_tol), ("scaled_mde3", mde_tol)):
        err = float(np.abs(out[k] - c["head." + k]).max())
        print(f"head.{k}: forward max |hip - captured| {err:.3g}, {err / tol:.3g} of the tolerance {tol:.3g}")
        assert err <= tol, k
    # the composed taps: the stereo block's volume is itself recomputed here (the maps' rounding goes through the
    # mirror detector's two gain-20 sigmoids into the mask and is multiplied by volume values up to 61: 3.6e-5
    # measured), so the lookup's own tolerance does not apply; the float64 head and the reference's own error do
    for b in range(2):
        for n in range(meta["iters"]):
            k, want = f"taps.{b}.{n}", o64[f"taps.{b}.{n}"]
            e_ref, err = float(np.abs(c[f"s7.{b}.{n}.taps"] - want).max()), float(np.abs(out[k] - want).max())
            print(f"head {k}: forward err {err:.3g}, e_ref {e_ref:.3g}, err / e_ref {err / e_ref:.3g}")
            assert out[k].shape == c[f"s7.{b}.{n}.taps"].shape and err <= 4 * e_ref, k
    for k in I.HEAD_GRADS:
        e_ref, err = I.e_ref(c, g64, k), float(np.abs(grads[k] - g64[k]).max())
        print(f"{k}: err {err:.3g}, e_ref {e_ref:.3g} ({e_ref / np.abs(g64[k]).max():.2g} of max |g|), err / e_ref {err / e_ref:.3g}")
        assert err <= 4 * e_ref, k

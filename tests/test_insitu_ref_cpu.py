"""The project's restatements are the reference's: every restatement the HIP backward kernels were built to
(tests/diffops_ref.py, lsq_lrc_ref.py, corr_autograd_ref.py, volume_stage_ref.py's truncation, blocks.Hourglass's
torch path) reproduces the outputs and the input gradients the REFERENCE's own autograd produced in its training
forward and backward (tests/golden/make_golden_insitu.py), from the captured inputs and output gradients, site by
site and as the composed volume head of stereoanywhere.py:174-271.

Per tensor, with cap the capture (float32), r32 / r64 the restatement in float32 / float64:

  e_ref = max |cap - r64|   the reference's own float32 error; tests/test_gpu_insitu.py allows the HIP drop-ins
                            4 e_ref, the suite's standing criterion;
  e_32  = max |r32 - r64|   the restatement's.

The check: e_ref <= 4 e_32, the standing criterion with the capture as the subject.  Two float32 evaluations of one
formula differ from its float64 evaluation by rounding alone, in whatever order they sum; a restatement with other
semantics (a detach, a sign, a permute, a missing consumer) moves e_ref by a fraction of the tensor's magnitude, 10^3
to 10^6 times e_32, while e_32 stays what it was.  Where the restatement is float64 numpy only (the correlation
path) the capture is held to that path's derived rounding bound instead, and the fraction used is printed."""
import copy
import os

import numpy as np
import pytest
import torch

import insitu_util as I
from fixtures_util import GOLDEN

U = I.U


@pytest.fixture(scope="module")
def cap():
    fix, meta = I.load()
    c = dict(fix)
    for s in I.S3_RUNS:
        c.update(I.s3_captured_sums(fix, s))
    c["s4.fused.g_d2"], c["s4.fused.g_d3"] = fix["s4.lrc0.g_d2"], fix["s4.lrc0.g_d3"]   # the same tensors' gradients
    c.update(I.head_captured(fix))
    return c, meta


def hold(cap, r32, r64, keys=None):
    for k in sorted(r64 if keys is None else keys):
        c = np.asarray(cap[k], np.float64)
        assert c.shape == r64[k].shape, k
        e_ref, e_32, mag = np.abs(c - r64[k]).max(), np.abs(r32[k] - r64[k]).max(), np.abs(r64[k]).max()
        same = "the same bits" if np.array_equal(cap[k], r32[k].astype(np.float32)) else f"max |cap - r32| {np.abs(c - r32[k]).max():.3g}"
        print(f"{k}: e_ref {e_ref:.3g} ({e_ref / mag:.2g} of max |ref|), e_32 {e_32:.3g}, e_ref / e_32 "
              f"{e_ref / max(e_32, 1e-300):.3g}; {same}")
        assert mag > 0, k
        assert e_ref <= 4 * e_32, k


def test_fixture_files(cap):
    """Every file within the size of the largest fixture committed before them; floats, finite, the gradients
    non-zero; the geometry the GPU tests are written for."""
    c, meta = cap
    fix, _ = I.load()
    largest_earlier = os.path.getsize(os.path.join(GOLDEN, "tiny_64x128_it4.npz"))
    on_disk = sorted(n for n in os.listdir(GOLDEN) if n.startswith("insitu_") and n.endswith(".npz"))
    assert on_disk == sorted(meta["files"])          # the index names exactly the files (load() checks their keys)
    for name in meta["files"]:
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= min(largest_earlier, 1 << 20), name
    for k, v in fix.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
        if ".g_" in k or k.startswith("s2.p."):
            assert np.abs(v).max() > 0, k
    assert (meta["B"], meta["H"], meta["W"], meta["iters"]) == (2, 64, 128, 4)
    assert fix["s3.dL.vol"].shape == (2, 1, 16, 32, 32) and fix["s1.out"].shape == (2, 16, 32, 1, 32)


def test_fixture_exercises_the_edges(cap):
    """What the capture script checks before it writes, on what was committed."""
    c, meta = cap
    W2 = c["s3.dL.vol"].shape[-1]
    xs = np.concatenate([c[f"s7.0.{n}.coords"][:, 0].ravel() for n in range(meta["iters"])])
    assert ((xs < 0) | (xs >= W2)).any()
    peak = c["s3.dL.vol"][:, 0].argmax(-1)
    assert ((peak == 0) | (peak == W2 - 1)).any()
    import lsq_lrc_ref
    B = meta["B"]
    for b in range(B):
        keep = lsq_lrc_ref.band(I.t(c["s5.disp"].reshape(B, -1)[b]))[2].numpy()
        assert keep.sum() >= 2 and np.ptp(np.abs(c["s5.mde"].reshape(B, -1)[b][keep])) > 0
    # the masked volume is mostly exact zeros; the upstream gradients span orders of magnitude
    assert (c["s2.x"] == 0).mean() > 0.8
    g = np.abs(c["s7.0.g_fullcorr"])
    assert g.max() / g[g > 0].min() > 1e4


def test_s1_corr_volume(cap):
    """CorrBlock1D.corr (:135): (K + 3) u sum |terms| (tests/test_gpu_corr_backward.py::test_corr_volume_backward),
    K the length of the sum: C for the volume, W2 / W1 for the gradients of fmap2 / fmap3."""
    c, _ = cap
    r64, mag = I.site_s1(c)
    B, C, H, W1 = c["s1.f2"].shape
    for k, K in (("s1.out", C), ("s1.g_f2", c["s1.f3"].shape[3]), ("s1.g_f3", W1)):
        err, bound = np.abs(c[k].astype(np.float64) - r64[k]), (K + 3) * U * mag[k]
        print(f"{k}: e_ref {err.max():.3g}, largest fraction of the bound {(err[bound > 0] / bound[bound > 0]).max():.3g}")
        assert np.all(err <= bound), k
        assert np.abs(r64[k]).max() > 0


@pytest.mark.parametrize("s", I.S3_RUNS)
def test_s3_softargmin(cap, s):
    """The run proper, and the run with the classifiers' weights multiplied by 64: one sharp peak on most lines,
    confidences up to 1, which the seeded classifiers do not give."""
    c, _ = cap
    hold(c, I.site_s3(c, torch.float32, s), I.site_s3(c, torch.float64, s))
    if s == "s3p":
        peak = torch.softmax(I.t(c["s3p.dL.vol"][:, 0]), -1).amax(-1)
        assert float(peak.median()) > 0.5 and max(c["s3p.cL.out"].max(), c["s3p.cR.out"].max()) > 0.9


def test_s4_softlrc_and_product(cap):
    c, meta = cap
    hold(c, I.site_s4(c, meta, torch.float32), I.site_s4(c, meta, torch.float64))
    # autograd adds nothing between softlrc and the products: the gradients the products send to their second
    # operand are the ones that arrive at softlrc's outputs
    assert np.array_equal(c["s4.lrc0.g_s2"], c["s4.and0.g_y"]) and np.array_equal(c["s4.lrc0.g_s3"], c["s4.and1.g_y"])
    assert "s4.lrc1.g_s2" not in c and "s4.lrc1.g_d2" not in c      # :199 feeds the detached truncation only


def test_s5_weighted_lsq(cap):
    c, _ = cap
    hold(c, I.site_s5(c, torch.float32), I.site_s5(c, torch.float64))


def test_s6_truncation(cap):
    """The mask and the product against volume_stage_ref at its own measured tolerance (4 E |ref| + 2^-126 is what
    the GPU tests allow; the reference's fp32 gets E), the volume's gradient by the rule above; nothing flows into
    the two maps (:203 detaches the mask)."""
    import volume_stage_ref as R
    c, meta = cap
    r32, r64 = I.site_s6(c, meta, torch.float32), I.site_s6(c, meta, torch.float64)
    for k in ("s6.mask", "s7.0.fullcorr"):
        dev = R.rel_deviation(I.t(c[k]), torch.from_numpy(r64[k]))
        print(f"{k}: relative deviation {dev:.3g}, {dev / R.E:.3g} of E")
        assert dev <= R.E, k
    hold(c, r32, r64)
    assert not any(k in c for k in ("s6.g_mask", "s6.g_disp", "s6.g_conf"))


def test_s7_lookups(cap):
    """CorrBlock1D.__init__ / __call__ of both blocks over the loop, against corr_autograd_ref with coefficients from
    the float64 coordinates.  The reference forms its sampling position in fp32 through grid_sample's normalised
    coordinates (x / 2^l + t, 2 x / (W - 1) - 1, ((x + 1) / 2) (W - 1): four roundings of values up to 2 on a scale
    of W / 2 and two of values up to W: 6 u W), so the position, and with it each of the two coefficients, is within
    8 u W2 of the float64 one.  A tap is e v0 + w v1 of pooled cells (L - 1 averages, 3 roundings of its own), both
    coefficients off: per tap |err| <= (L + 3) u mag + 8 u W2 mag_1.  A fullcorr gradient cell sums at most 4 scattered
    terms per iteration and the fold's L levels: |err| <= (5 iters + L + 8) u mag + 8 u W2 mag_1.  mag is the sum of the
    absolute terms (the existing correlation bounds' magnitude) and mag_1 the same sum with every non-zero coefficient
    replaced by 1 (|v0| + |v1| for a tap)."""
    import corr_autograd_ref as ref
    c, meta = cap
    L, iters = meta["corr_levels"], meta["iters"]
    r64, mag = I.site_s7(c, meta)
    ones = [(A != 0).astype(np.float64) for A in I.lookup_matrices(c, meta)]
    for b in range(2):
        full = c[f"s7.{b}.fullcorr"]
        W2 = full.shape[-1]
        apyr = ref.pyramid_forward(np.abs(full).reshape(-1, W2), L)
        for n in range(iters):
            k = f"s7.{b}.{n}.taps"
            pair = I._taps(ref.lookup_forward(ones[n], apyr), c[k])
            err, bound = np.abs(c[k] - r64[k]), (L + 3) * U * mag[k] + 8 * U * W2 * pair
            print(f"{k}: e_ref {err.max():.3g}, largest fraction of the bound {(err[bound > 0] / bound[bound > 0]).max():.3g}")
            assert np.all(err <= bound), k
        k = f"s7.{b}.g_fullcorr"
        m1 = sum(ref.lookup_backward(A1, np.abs(c[f"s7.{b}.{n}.g_taps"])) for n, A1 in enumerate(ones))
        bound = (5 * iters + L + 8) * U * mag[k] + 8 * U * W2 * ref.pyramid_backward(m1, W2, L).reshape(full.shape)
        err = np.abs(c[k] - r64[k])
        print(f"{k}: e_ref {err.max():.3g}, largest fraction of the bound {(err[bound > 0] / bound[bound > 0]).max():.3g}")
        assert np.all(err <= bound) and np.abs(r64[k]).max() > 0
        assert np.all(c[k][bound == 0] == 0)
    # the mono block's volume is the classifier's, the stereo block's the truncated product
    assert np.array_equal(I.volume5(c["s7.1.fullcorr"]), c["s3.dL.vol"])


def test_s8_convex_upflow(cap):
    c, meta = cap
    hold(c, I.site_s8(c, meta, torch.float32), I.site_s8(c, meta, torch.float64))


def test_s2_hourglass(cap):
    """blocks.Hourglass's torch path with the seeded weights: the output, the gradients of the masked volume and of
    the feature maps, every parameter's gradient; the parameters of the reference's dead branches have none on
    either side."""
    c, meta = cap
    hg = I.hourglass_module(meta)
    r32 = I.run_hourglass(c, copy.deepcopy(hg), torch.float32)
    r64 = I.run_hourglass(c, copy.deepcopy(hg), torch.float64)
    dead = sorted(k for k, v in r64.items() if v is None)
    assert dead == sorted(["s2.g_fl3", "s2.g_fr3"] + ["s2.p." + n for n in meta["hourglass_dead_parameters"]])
    assert not any(k in c for k in dead)
    live = sorted(k for k, v in r64.items() if v is not None)
    assert live == sorted(k for k in c if k.startswith("s2.") and (k == "s2.out" or ".g_" in k or k.startswith("s2.p."))
                          and k != "s2.g_out")
    hold(c, r32, r64, live)


def test_head(cap):
    """stereoanywhere.py:174-271 composed from the restatements as INTEGRATION.md wires the drop-ins: the six
    returned coarse entries, the mirror confidence, and the total gradients at the three input volumes from the
    captured gradients of the head's outputs (the coarse entries and every iteration's taps)."""
    c, meta = cap
    o32, g32 = I.run_head(I.RefOps(torch.float32), c, meta, torch.float32)
    o64, g64 = I.run_head(I.RefOps(torch.float64), c, meta, torch.float64)
    outs = {"head." + k: v for k, v in o64.items() if k in I.HEAD_OUTPUTS}
    hold(c, {"head." + k: v for k, v in o32.items()}, outs)
    hold({"mirror": c["s6.conf"], "smde2_lr": c["s6.disp"]}, o32, {k: o64[k] for k in ("mirror", "smde2_lr")})
    hold(c, g32, g64)

"""The volume stage on the GPU (csrc/volume_stage.hip through ops and diffops) against the project's
own restatement (tests/volume_stage_ref.py) and the reference's captured volumes
(tests/golden/volume_stage.npz).  Roll, noise and none are exact (torch.equal); the zero kind and every
truncated result are held to 4 E |ref64| + 2^-126 with E measured on the CPU
(tests/test_volume_stage_ref_cpu.py), never taken from the kernels."""
import functools
import json

import pytest
import torch

import volume_stage_ref as R
from fixtures_util import load_fixture
from stereoanywhere_amd import _native as N, diffops, ops
from stereoanywhere_amd.diffops import VolumeCorruption

pytestmark = pytest.mark.gpu
dev = "cuda"

# (B, H, W1, W2): less than a vector; scalar tail and odd rows; aligned; a row longer than one
# 256-lane pass; W1 != W2 (roll and noise only)
SQUARE = [(1, 1, 5, 5), (2, 3, 37, 37), (1, 2, 64, 64), (1, 2, 260, 260)]
SHAPES = SQUARE + [(2, 2, 40, 24)]
BINS = [(4, 0), (4, 3), (3, 0), (3, 2)]   # first and last bin; 3: a threshold that is no power of two


@functools.lru_cache(maxsize=None)
def case(shape):
    """The seeded CPU inputs of a shape, built once and never modified."""
    return R.random_case(sum(shape), *shape)


def gpu(c, *keys):
    return [c[k].to(dev) for k in keys]


def run(c, kind="none", nbins=1, bin=0, shift=1, noise=None, trunc=None, out=None, volume=None):
    """ops.volume_stage on the case's tensors -> CPU result."""
    vol = c["volume"].to(dev) if volume is None else volume
    kw = dict(kind=kind, nbins=nbins, bin=bin, shift=shift, out=out)
    if kind != "none":
        kw["mde"] = c["mde"].to(dev)
    if kind == "noise":
        kw["noise"] = (c["noise"] if noise is None else noise).float().to(dev)
    if kind == "zero":
        kw["peak"] = ops.volume_peak(vol)
    if trunc is not None:
        kw.update(trunc_disp=c["disp"].to(dev), trunc_conf=c["conf"].to(dev), atten=trunc)
    got = ops.volume_stage(vol, **kw)
    torch.cuda.synchronize()
    return got.cpu()


def want(c, kind="none", nbins=1, bin=0, shift=1, trunc=None, dtype=torch.float32):
    return R.stage(c["volume"], kind, c["mde"], nbins, bin, shift, c["noise"],
                   None if trunc is None else (c["disp"], c["conf"], trunc), dtype)


@pytest.mark.parametrize("shape", SHAPES)
def test_roll_noise_none_are_exact(shape):
    c = case(shape)
    W1 = shape[2]
    assert torch.equal(run(c), c["volume"])
    for nbins, b in BINS:
        m = R.bin_mask(c["mde"], nbins, b)
        assert 0 < int(m.sum()) < m.numel() or shape == SHAPES[0]
        for shift in (1, W1 - 1, W1):
            assert torch.equal(run(c, "roll", nbins, b, shift), want(c, "roll", nbins, b, shift)), (nbins, b, shift)
        assert torch.equal(run(c, "noise", nbins, b), want(c, "noise", nbins, b)), (nbins, b)
    # shift == W1 is the identity
    assert torch.equal(run(c, "roll", 4, 0, W1), c["volume"])


def test_mask_edges_all_and_none():
    """mde exactly 0, 0.25, 0.5, 1.0 and a negative value (the first five pixels of the case's first
    row): bins are half open, 1.0 and negatives are in none; then an all-masked and a none-masked map."""
    c = dict(case((1, 1, 5, 5)))
    assert c["mde"].flatten().tolist() == [0.0, 0.25, 0.5, 1.0, pytest.approx(-0.3)]
    two = torch.full_like(c["noise"], 2.0)
    for b, rows in ((0, [0]), (1, [1]), (2, [2]), (3, [])):
        got = run(c, "noise", 4, b, noise=two)
        exp = c["volume"].clone()
        exp[0, 0, 0, rows] *= 2.0
        assert torch.equal(got, exp), b
    big = dict(case((2, 3, 37, 37)))
    for value, masked in ((0.1, True), (1.0, False), (-0.5, False)):
        big["mde"] = torch.full_like(big["mde"], value)
        for kind in ("roll", "noise"):
            got = run(big, kind, 4, 0, 5)
            exp = want(big, kind, 4, 0, 5)
            assert torch.equal(got, exp)
            assert torch.equal(got, big["volume"]) != masked
        R.assert_close(run(big, "zero", 4, 0), want(big, "zero", 4, 0, dtype=torch.float64), f"zero, mde {value}")


@pytest.mark.parametrize("atten", [0.9, 0.1])
@pytest.mark.parametrize("shape", SQUARE)
def test_zero_and_truncated_within_measured_tolerance(shape, atten):
    c = case(shape)
    W1 = shape[2]
    R.assert_close(run(c, trunc=atten), want(c, trunc=atten, dtype=torch.float64), "truncated")
    ones = dict(c, volume=torch.ones_like(c["volume"]))
    R.assert_close(run(ones, trunc=atten), R.trunc_factor(c["disp"], c["conf"], atten, W1, torch.float64), "factor")
    for nbins, b in BINS:
        for trunc in (None, atten):
            R.assert_close(run(c, "zero", nbins, b, trunc=trunc), want(c, "zero", nbins, b, trunc=trunc, dtype=torch.float64),
                           f"zero {nbins}/{b} trunc {trunc}")
        R.assert_close(run(c, "roll", nbins, b, W1 - 1, trunc=atten),
                       want(c, "roll", nbins, b, W1 - 1, trunc=atten, dtype=torch.float64), f"roll {nbins}/{b} truncated")
        R.assert_close(run(c, "noise", nbins, b, trunc=atten),
                       want(c, "noise", nbins, b, trunc=atten, dtype=torch.float64), f"noise {nbins}/{b} truncated")


def test_in_place():
    c = case((2, 3, 37, 37))
    for kw in (dict(kind="noise", nbins=4, bin=0), dict(kind="zero", nbins=4, bin=3), dict(trunc=0.9),
               dict(kind="noise", nbins=4, bin=1, trunc=0.1)):
        vol = c["volume"].to(dev)
        assert torch.equal(run(c, out=vol, volume=vol, **kw), run(c, **kw)), kw
    g = c["volume"].to(dev)
    d, t = gpu(c, "disp", "conf")
    fresh = ops.volume_truncate_backward(g, d, t, 0.9)
    assert ops.volume_truncate_backward(g, d, t, 0.9, out=g) is g
    assert torch.equal(g, fresh) and torch.equal(fresh.cpu(), run(c, trunc=0.9))


@pytest.mark.parametrize("n", [25, 2 * 3 * 37 * 37, 2 * 260 * 260, 1024 * 4096 + 4099])
def test_peak_equals_torch_max_on_bits(n):
    """Random data, an all-negative volume, the maximum in the scalar tail, and one NaN in the last
    element; n: less than a block, odd counts, and more than the 1024 partials cover in one step."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    for v in (x, -x.abs() - 1.0, torch.cat([x[:-1], x.max().view(1) + 1.0])):
        got = ops.volume_peak(v.to(dev)).cpu()
        assert got.shape == (1,) and torch.equal(got.view(torch.int32), v.max().view(1).view(torch.int32))
    nan = x.clone()
    nan[-1] = float("nan")
    assert torch.isnan(ops.volume_peak(nan.to(dev)).cpu()).all()
    nan[-1], nan[n // 2] = 0.0, float("nan")
    assert torch.isnan(ops.volume_peak(nan.to(dev)).cpu()).all()


def test_nan_volume_zero_kind():
    """torch.max of a volume with a NaN is NaN: every masked cell becomes NaN, the rest is untouched."""
    c = dict(case((2, 3, 37, 37)))
    c["volume"] = c["volume"].clone()
    c["volume"][-1, -1, -1, -1, -1] = float("nan")
    got = run(c, "zero", 4, 1)
    m = R.bin_mask(c["mde"], 4, 1).expand_as(got)
    assert 0 < int(m.sum()) < m.numel()
    assert torch.isnan(got[m]).all()
    assert torch.equal(got[~m].view(torch.int32), c["volume"][~m].view(torch.int32))


@functools.lru_cache(maxsize=None)
def golden():
    return load_fixture("volume_stage.npz")


@pytest.mark.parametrize("name", ["none", "stereo_roll", "stereo_noise", "stereo_zero", "mono_roll", "mono_noise",
                                  "mono_zero"])
def test_golden_cases_reproduce_the_reference(name):
    fix = golden()
    t = {k: torch.from_numpy(fix[k]).to(dev) for k in ("stereo_in", "mono_in", "mde2_lowres", "trunc_disp", "trunc_conf")}
    plan = json.loads(str(fix[f"{name}.plan"]))
    plan = None if plan is None else VolumeCorruption(*plan)
    noise = torch.from_numpy(fix[f"{name}.noise"]).to(dev) if f"{name}.noise" in fix else None
    stereo, mono = diffops.volume_stage(t["stereo_in"], t["mono_in"], t["mde2_lowres"], plan,
                                        (t["trunc_disp"], t["trunc_conf"], float(fix["trunc_atten"])), noise)
    torch.cuda.synchronize()
    ref_s, ref_m = (torch.from_numpy(fix[f"{name}.{k}"]) for k in ("stereo_out", "mono_out"))
    # the stereo volume is truncated in every case: the measured tolerance, against the reference's fp32
    # capture and against the float64 restatement of the same inputs (which the capture is within E of)
    cpu = {k: v.cpu() for k, v in t.items()}
    kw = {}
    if plan is not None:
        kw = dict(kind=plan.kind, mde=cpu["mde2_lowres"], nbins=4, bin=plan.bin, shift=max(plan.shift, 1),
                  noise=None if noise is None else noise.cpu())
    trunc = (cpu["trunc_disp"], cpu["trunc_conf"], float(fix["trunc_atten"]))
    s_kw = kw if plan is not None and plan.target == "stereo" else {}
    m_kw = kw if plan is not None and plan.target == "mono" else {}
    s64 = R.stage(cpu["stereo_in"], trunc=trunc, dtype=torch.float64, **s_kw)
    m64 = R.stage(cpu["mono_in"], dtype=torch.float64, **m_kw)
    assert R.rel_deviation(ref_s, s64) <= R.E and R.rel_deviation(ref_m, m64) <= R.E   # the capture itself
    R.assert_close(stereo, s64, f"{name} stereo vs float64")
    R.assert_close(stereo, ref_s.double(), f"{name} stereo vs the capture")
    if plan is not None and plan.target == "mono" and plan.kind == "zero":
        R.assert_close(mono, m64, f"{name} mono vs float64")
        R.assert_close(mono, ref_m.double(), f"{name} mono vs the capture")
    else:
        assert torch.equal(mono.cpu(), ref_m)
    if plan is None or plan.target == "stereo":
        assert mono is t["mono_in"]


def test_fused_equals_composition_on_bits():
    c = case((2, 3, 37, 37))
    vol, mono, mde, noise, d, t = gpu(c, "volume", "volume", "mde", "noise", "disp", "conf")
    for kind in ("roll", "noise", "zero"):
        for atten in (0.9, 0.1):
            plan = VolumeCorruption("stereo", kind, 2, 7 if kind == "roll" else 0)
            fused, m_out = diffops.volume_stage(vol, mono, mde, plan, (d, t, atten), noise)
            two = diffops.truncate_volume(diffops.corrupt_volume(vol, mde, plan, noise), d, t, atten)
            assert m_out is mono
            assert torch.equal(fused.view(torch.int32), two.view(torch.int32)), (kind, atten)
    plan = VolumeCorruption("mono", "noise", 0, 0)
    s_out, m_out = diffops.volume_stage(vol, mono, mde, plan, None, noise)
    assert s_out is vol and torch.equal(m_out, diffops.corrupt_volume(mono, mde, plan, noise))
    s_out, m_out = diffops.volume_stage(vol, mono)
    assert s_out is vol and m_out is mono


def test_corrupt_volume_inputs_and_default_noise():
    c = case((2, 2, 40, 24))
    vol, mde, noise = gpu(c, "volume", "mde", "noise")
    plan = VolumeCorruption("stereo", "noise", 1, 0)
    exp = diffops.corrupt_volume(vol, mde, plan, noise)
    assert exp.dtype == torch.float32 and not exp.requires_grad and exp.data_ptr() != vol.data_ptr()
    assert torch.equal(exp.cpu(), want(c, "noise", 4, 1))
    # fp32 noise of the same values, a [B,1,H,W1] noise, a non-contiguous volume, a volume that requires grad
    assert torch.equal(diffops.corrupt_volume(vol, mde, plan, noise.float()), exp)
    assert torch.equal(diffops.corrupt_volume(vol, mde, plan, noise.squeeze(4)), exp)
    strided = vol.transpose(3, 4).contiguous().transpose(3, 4)
    assert not strided.is_contiguous() and torch.equal(diffops.corrupt_volume(strided, mde, plan, noise), exp)
    out = diffops.corrupt_volume(vol.clone().requires_grad_(), mde, plan, noise)
    assert out.grad_fn is None and not out.requires_grad
    # an fp16 volume is cast with .float()
    half = diffops.corrupt_volume(vol.half(), mde, plan, noise)
    assert half.dtype == torch.float32 and torch.equal(half, diffops.corrupt_volume(vol.half().float(), mde, plan, noise))
    # noise=None draws what the reference's rand_like of its fp16 mask draws: fp16, [B,1,H,W1,1]
    torch.manual_seed(11)
    drawn = diffops.corrupt_volume(vol, mde, plan)
    after = torch.rand(3, device=dev)
    torch.manual_seed(11)
    n16 = torch.rand((2, 1, 2, 40, 1), dtype=torch.float16, device=dev)
    assert torch.equal(after, torch.rand(3, device=dev))   # the same generator stream was consumed
    assert torch.equal(drawn, diffops.corrupt_volume(vol, mde, plan, n16))
    # n_masks other than the default
    assert torch.equal(diffops.corrupt_volume(vol, mde, VolumeCorruption("stereo", "noise", 2, 0), noise, n_masks=3).cpu(),
                       want(c, "noise", 3, 2))


def test_refusals():
    c = case((2, 2, 40, 24))
    vol, mde, noise, d, t = gpu(c, "volume", "mde", "noise", "disp", "conf")
    sq = case((2, 3, 37, 37))
    svol, smde, sd, st = gpu(sq, "volume", "mde", "disp", "conf")
    roll = VolumeCorruption("stereo", "roll", 0, 3)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        diffops.corrupt_volume(c["volume"], mde, roll)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        diffops.truncate_volume(svol, sq["disp"], st)
    with pytest.raises(RuntimeError, match=r"volume must be \[B,1,H,W1,W2\]"):
        diffops.corrupt_volume(vol[:, 0], mde, roll)
    with pytest.raises(RuntimeError, match=r"mde_lowres must be \[B,1,H,W1\]"):
        diffops.corrupt_volume(vol, mde[:, :, :, :-1], roll)
    with pytest.raises(RuntimeError, match="needs mde_lowres"):
        diffops.corrupt_volume(vol, None, roll)
    with pytest.raises(RuntimeError, match="plan is None"):
        diffops.corrupt_volume(vol, mde, None)
    with pytest.raises(RuntimeError, match="kind must be 'roll', 'noise' or 'zero'"):
        diffops.corrupt_volume(vol, mde, VolumeCorruption("stereo", "blur", 0, 0))
    with pytest.raises(RuntimeError, match="target must be 'stereo' or 'mono'"):
        diffops.volume_stage(vol, vol, mde, VolumeCorruption("left", "roll", 0, 1))
    with pytest.raises(RuntimeError, match=r"bin must be 0\.\.3"):
        diffops.corrupt_volume(vol, mde, VolumeCorruption("stereo", "noise", 4, 0), noise)
    for shift in (0, 41):
        with pytest.raises(RuntimeError, match=r"shift must be 1\.\.W1 = 40"):
            diffops.corrupt_volume(vol, mde, VolumeCorruption("stereo", "roll", 0, shift))
    with pytest.raises(RuntimeError, match="'zero' corruption needs W1 == W2"):
        diffops.corrupt_volume(vol, mde, VolumeCorruption("stereo", "zero", 0, 0))
    with pytest.raises(RuntimeError, match="truncation needs W1 == W2"):
        diffops.truncate_volume(vol, d, t, 0.9)
    with pytest.raises(RuntimeError, match=r"disp_left must be \[B,1,H,W1\]"):
        diffops.truncate_volume(svol, sd[:1], st, 0.9)
    # the library's own refusals, by their messages
    with pytest.raises(N.NativeError, match="SA_VOLAUG_ROLL cannot run in place"):
        ops.volume_stage(vol, "roll", mde, 4, 0, 3, out=vol)
    with pytest.raises(N.NativeError, match="shift must be 1..W1"):
        ops.volume_stage(vol, "roll", mde, 4, 0, 41)
    with pytest.raises(N.NativeError, match="bin must be 0..nbins-1"):
        ops.volume_stage(vol, "noise", mde, 3, 3, noise=noise.float())
    with pytest.raises(N.NativeError, match="needed by SA_VOLAUG_NOISE"):
        ops.volume_stage(vol, "noise", mde, 4, 0)
    with pytest.raises(N.NativeError, match="needed by SA_VOLAUG_ZERO"):
        ops.volume_stage(svol, "zero", smde, 4, 0)
    with pytest.raises(N.NativeError, match="SA_VOLAUG_ZERO needs W1 == W2"):
        ops.volume_stage(vol, "zero", mde, 4, 0, peak=ops.volume_peak(vol))
    with pytest.raises(N.NativeError, match="trunc_disp and trunc_conf go together"):
        ops.volume_stage(svol, trunc_disp=sd)
    with pytest.raises(N.NativeError, match="the truncation needs W1 == W2"):
        ops.volume_stage(vol, trunc_disp=d, trunc_conf=t)
    with pytest.raises(RuntimeError, match="kind must be one of"):
        ops.volume_stage(vol, "blur")
    with pytest.raises(RuntimeError, match="must be float32"):
        ops.volume_stage(vol.half())
    with pytest.raises(RuntimeError, match="out must have the volume's shape"):
        ops.volume_stage(vol, out=svol)
    torch.cuda.synchronize()

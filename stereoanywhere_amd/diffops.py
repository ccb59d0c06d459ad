"""Differentiable drop-ins for the reference's soft-argmin / entropy-confidence functions, its
convex up-sampling, its soft left-right consistency and its weighted least-squares scale / shift
(models/stereoanywhere/utils/utils.py:97-198, 345-384).

``estimate_left_disparity``, ``estimate_right_disparity``, ``estimate_left_confidence``,
``estimate_right_confidence``, ``convex_upflow``, ``softlrc`` and ``weighted_lsq`` keep the
reference's names and signatures; ``softargmin_conf`` is the joint form (all four maps of a disparity
and a confidence volume from one forward and one backward) and the one to prefer: four separate calls
are four forwards, four backwards and two volume-sized additions by autograd.  ``softlrc_conf`` is
``fuzzy_and(conf, softlrc)`` of both maps in one launch, as the model's forward uses it.

With grad mode on and an input that requires grad the functions run as the autograd functions below:
the forward is the inference kernel (``ops.softargmin_conf`` / ``ops.convex_upsample`` /
``ops.softlrc`` / the one-launch ``ops.weighted_lsq``, so the same bits), the backward a
deterministic HIP adjoint (csrc/diffops_backward.hip, csrc/lsq_backward.hip) that recomputes the
forward from the saved inputs; nothing but the inputs is saved, plus for ``weighted_lsq`` its two
outputs and a record of six doubles per sample (the band thresholds, the normal-equation sums, the
branch taken).  Otherwise they make the plain ``ops`` calls and return tensors without a ``grad_fn``.
Double backward is not built.

``weighted_lsq`` gives all-zero gradients for a sample whose kept mono values are all equal or whose
band is empty: the forward takes its minimum-norm / zero branch there, and the reference's GPU
``lstsq`` assumes full rank, so there is nothing to match.  The band thresholds are constants, as in
the reference, which only compares against them.

``volume_stage`` is the stage between the aggregated volumes and the two ``corr_block(...)``
constructors of the training forward (stereoanywhere.py:214-255): ``draw_volume_corruption`` makes the
reference's draws, ``corrupt_volume`` applies one volume-corruption branch (detached, as the reference
detaches it) and ``truncate_volume`` is the truncation multiply, differentiable with respect to the
volume and saving the two maps its factor is recomputed from (csrc/volume_stage.hip).

``volume_close`` is the close of a training-time hourglass layer, InstanceNorm3d + LeakyReLU (+ the
DoubleFeatureAtt gate), on a volume a torch conv produced: differentiable with respect to the volume and
both gate maps, saving the volume, the maps and the statistics (csrc/volume_close.hip);
``hourglass_forward`` is the reference's ``Hourglass.forward`` built on it.

``upcat_conv`` is a join of that hourglass, the 1x1x1 conv over ``cat`` of a volume and a trilinearly
up-sampled coarser one, as ``Wa . skip + up(Wu . low)``: differentiable with respect to both volumes and the
weight, saving exactly those three (csrc/upcat_backward.hip); ``hourglass_forward(joins="hip")`` uses it.

``conv3d_k3`` is a stride-1 3x3x3 conv of that hourglass with equal channel counts (8, 16 or 32): the inference
split-f16 MFMA kernel forward and, with the flipped kernel, for the data gradient, a HIP weight gradient
(csrc/conv3d_backward.hip), per-sample power-of-two scales where an operand has no known range; saves exactly the
input and the weight; ``hourglass_forward(convs="hip")`` uses it.

Floating inputs that are not fp32 (fp16 / bf16 activations under ``torch.autocast``) are cast with
``.float()``: a torch op, so the gradient arrives at the caller's tensor in its own dtype.  There is
no CPU path.
"""
from __future__ import annotations

import random
from typing import NamedTuple, Optional, Sequence

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .corr import _wants_grad


def _on_gpu(t: torch.Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} must be on the GPU (the HIP path has no CPU fallback), got {t.device}")
    if not t.is_floating_point():
        raise RuntimeError(f"{name} must be a floating-point tensor, got {t.dtype}")


# ------------------------------------------------------------------------------- soft-argmin
def _volume(v: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    """[B,1,H,W1,W2] in fp32 with W1 or W2 at stride 1 (a view where the input already is)."""
    if v is None:
        return None
    _on_gpu(v, name)
    if v.dim() != 5 or v.shape[1] != 1:
        raise RuntimeError(f"{name} must be [B,1,H,W1,W2], got {tuple(v.shape)}")
    if v.shape[3] < 2 or v.shape[4] < 2:
        raise RuntimeError(f"{name}: W1 and W2 must be at least 2, got {tuple(v.shape)}")
    v = v.float()
    if v.stride(4) != 1 and v.stride(3) != 1:
        v = v.contiguous()
    return v


def _geometry(v: torch.Tensor):
    B, _, H, W1, W2 = v.shape
    return (v.stride(0), v.stride(2), v.stride(3), v.stride(4)), (B, H, W1, W2)


def _forward_maps(vol_disp, vol_conf):
    """The inference kernel on either or both volumes -> (dL, dR, cL, cR), [B,1,H,W] each or None."""
    strides, dims = _geometry(vol_disp if vol_disp is not None else vol_conf)
    return ops.softargmin_conf_maps(vol_disp, vol_conf, strides, dims)


class _SoftArgminConfFn(torch.autograd.Function):
    """ops.softargmin_conf with ops.softargmin_conf_backward as its adjoint.  Saves the volumes only;
    an output nobody used arrives as a None gradient and is passed on as a null pointer."""

    @staticmethod
    def forward(ctx, vol_disp, vol_conf):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(vol_disp, vol_conf)
        return _forward_maps(vol_disp, vol_conf)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_dL, g_dR, g_cL, g_cR):
        vol_disp, vol_conf = ctx.saved_tensors
        need_d, need_c = ctx.needs_input_grad
        if not need_d:
            g_dL = g_dR = None
        if not need_c:
            g_cL = g_cR = None
        grads = [None if g is None else g.float().contiguous() for g in (g_dL, g_dR, g_cL, g_cR)]
        if all(g is None for g in grads):
            return None, None
        ref = vol_disp if vol_disp is not None else vol_conf
        strides, dims = _geometry(ref)
        return ops.softargmin_conf_backward(vol_disp, vol_conf, strides, dims, *grads)


def softargmin_conf(vol_disp: Optional[torch.Tensor], vol_conf: Optional[torch.Tensor]):
    """(estimate_left_disparity(vol_disp), estimate_right_disparity(vol_disp),
    estimate_left_confidence(vol_conf), estimate_right_confidence(vol_conf)) from one forward and one
    backward; volumes [B,1,H,W1,W2], either may be None (its two maps are None)."""
    vol_disp, vol_conf = _volume(vol_disp, "vol_disp"), _volume(vol_conf, "vol_conf")
    if vol_disp is None and vol_conf is None:
        raise RuntimeError("softargmin_conf: both volumes are None")
    if vol_disp is not None and vol_conf is not None:
        if vol_disp.shape != vol_conf.shape:
            raise RuntimeError(f"softargmin_conf: the volumes must have one shape, got {tuple(vol_disp.shape)} "
                               f"and {tuple(vol_conf.shape)}")
        if _geometry(vol_disp)[0] != _geometry(vol_conf)[0]:   # one set of strides per call
            vol_disp, vol_conf = vol_disp.contiguous(), vol_conf.contiguous()
    if _wants_grad(vol_disp, vol_conf):
        return _SoftArgminConfFn.apply(vol_disp, vol_conf)
    return _forward_maps(vol_disp, vol_conf)


def _padded(x: torch.Tensor, vol_pad: Sequence[int]) -> torch.Tensor:
    return x[:, :, :, vol_pad[0]:x.shape[3] - vol_pad[1]]


def estimate_left_disparity(corr_volume, vol_pad=[0, 0]):
    return _padded(softargmin_conf(corr_volume, None)[0], vol_pad)


def estimate_right_disparity(corr_volume, vol_pad=[0, 0]):
    return _padded(softargmin_conf(corr_volume, None)[1], vol_pad)


def estimate_left_confidence(corr_volume, logsumexp_eps=1e-3):
    return softargmin_conf(None, corr_volume)[2]


def estimate_right_confidence(corr_volume, logsumexp_eps=1e-3):
    return softargmin_conf(None, corr_volume)[3]


# ------------------------------------------------------------------------- convex up-sampling
class _ConvexUpFn(torch.autograd.Function):
    """ops.convex_upsample with ops.convex_upsample_backward as its adjoint.  Saves flow and mask."""

    @staticmethod
    def forward(ctx, flow, mask, factor, use_scale_factor):
        ctx.save_for_backward(flow, mask)
        ctx.geo = (factor, float(factor) if use_scale_factor else 1.0)
        return _upsample(flow, mask, factor, use_scale_factor)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        flow, mask = ctx.saved_tensors
        factor, scale = ctx.geo
        need_flow, need_mask = ctx.needs_input_grad[:2]
        if not (need_flow or need_mask):
            return None, None, None, None
        g_flow, g_mask = ops.convex_upsample_backward(flow, mask, grad.float().contiguous(), factor, scale,
                                                      need_flow, need_mask)
        return g_flow, g_mask, None, None


def _upsample(flow, mask, factor, use_scale_factor):
    # the kernel multiplies the flow by the factor; without use_scale_factor it gets flow / factor
    # (a power of two: both steps are exact)
    return ops.convex_upsample(flow if use_scale_factor else flow * (1.0 / factor), mask, factor)


def convex_upflow(flow, mask, n_downsample=2, use_scale_factor=True):
    """The reference's convex_upflow for one flow channel: flow [N,1,H,W], mask [N,9*f*f,H,W],
    f = 2**n_downsample <= 8 -> [N,1,f*H,f*W]."""
    _on_gpu(flow, "flow")
    _on_gpu(mask, "mask")
    if flow.dim() != 4 or mask.dim() != 4:
        raise RuntimeError(f"convex_upflow: flow and mask must be 4-D, got {tuple(flow.shape)} and {tuple(mask.shape)}")
    n, d, h, w = flow.shape
    if d != 1:
        raise RuntimeError(f"convex_upflow: flow has D = {d} channels; the HIP path up-samples D == 1 (the x flow) only")
    if not 0 <= n_downsample <= 3:
        raise RuntimeError(f"convex_upflow: n_downsample must be 0..3 (factor 1..8), got {n_downsample}")
    factor = 2 ** n_downsample
    if tuple(mask.shape) != (n, 9 * factor * factor, h, w):
        raise RuntimeError(f"convex_upflow: mask must be {(n, 9 * factor * factor, h, w)}, got {tuple(mask.shape)}")
    flow, mask = flow.float().contiguous(), mask.float().contiguous()
    if _wants_grad(flow, mask):
        return _ConvexUpFn.apply(flow, mask, factor, bool(use_scale_factor))
    return _upsample(flow, mask, factor, use_scale_factor)


# --------------------------------------------------------------- softLRC and weighted_lsq
class _SoftLrcFn(torch.autograd.Function):
    """ops.softlrc with ops.softlrc_backward as its adjoint.  Saves the maps only; an output nobody
    used arrives as a None gradient and is passed on as a null pointer."""

    @staticmethod
    def forward(ctx, d2, d3, conf2, conf3, lrc_th):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(d2, d3, conf2, conf3)
        ctx.lrc_th = lrc_th
        return ops.softlrc(d2, d3, conf2, conf3, lrc_th)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_s2, g_s3):
        d2, d3, conf2, conf3 = ctx.saved_tensors
        need = ctx.needs_input_grad[:4]
        if (g_s2 is None and g_s3 is None) or not any(need):
            return None, None, None, None, None
        g_s2, g_s3 = (None if g is None else g.float().contiguous() for g in (g_s2, g_s3))
        return (*ops.softlrc_backward(d2, d3, conf2, conf3, ctx.lrc_th, g_s2, g_s3, *need), None)


def _lrc_map(t: Optional[torch.Tensor], name: str, like: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    if t is None:
        return None
    _on_gpu(t, name)
    if t.dim() != 4 or t.shape[1] != 1:
        raise RuntimeError(f"{name} must be [B,1,H,W], got {tuple(t.shape)}")
    if like is not None and t.shape != like.shape:
        raise RuntimeError(f"{name} must have the shape of disp2 {tuple(like.shape)}, got {tuple(t.shape)}")
    return t.float().contiguous()


def _softlrc(disp2, disp3, conf2, conf3, lrc_th):
    d2 = _lrc_map(disp2, "disp2")
    d3, c2, c3 = (_lrc_map(t, n, d2) for t, n in ((disp3, "disp3"), (conf2, "conf2"), (conf3, "conf3")))
    if _wants_grad(d2, d3, c2, c3):
        return _SoftLrcFn.apply(d2, d3, c2, c3, float(lrc_th))
    return ops.softlrc(d2, d3, c2, c3, float(lrc_th))


def softlrc(disp2, disp3, lrc_th=1.0):
    """The reference's softlrc: disparity maps [B,1,H,W] -> (softlrc_disp2, softlrc_disp3)."""
    return _softlrc(disp2, disp3, None, None, lrc_th)


def softlrc_conf(disp2, disp3, conf2, conf3, lrc_th=1.0):
    """(fuzzy_and(conf2, softlrc_disp2), fuzzy_and(conf3, softlrc_disp3)) in one launch, forward and
    backward: the pair the reference's forward feeds to weighted_lsq and the mirror detector."""
    if conf2 is None or conf3 is None:
        raise RuntimeError("softlrc_conf: conf2 and conf3 must be given (softlrc is the form without them)")
    return _softlrc(disp2, disp3, conf2, conf3, lrc_th)


class _WeightedLsqFn(torch.autograd.Function):
    """ops.weighted_lsq_stats (the bits of ops.weighted_lsq) with ops.weighted_lsq_backward as its
    adjoint.  Saves the three maps, the two outputs and the per-sample record."""

    @staticmethod
    def forward(ctx, mde, disp, conf, q_lo, q_hi):
        ctx.set_materialize_grads(False)
        scale, shift, rec = ops.weighted_lsq_stats(mde, disp, conf, q_lo, q_hi)
        ctx.save_for_backward(mde, disp, conf, scale, shift, rec)
        return scale, shift

    @staticmethod
    @once_differentiable
    def backward(ctx, g_scale, g_shift):
        mde, disp, conf, scale, shift, rec = ctx.saved_tensors
        need = ctx.needs_input_grad[:3]
        if (g_scale is None and g_shift is None) or not any(need):
            return None, None, None, None, None
        g_scale, g_shift = (None if g is None else g.float().contiguous() for g in (g_scale, g_shift))
        return (*ops.weighted_lsq_backward(mde, disp, conf, scale, shift, rec, g_scale, g_shift, *need), None, None)


def weighted_lsq(mde, disp, conf, min_quantile=0.2, max_quantile=0.9):
    """The reference's weighted_lsq: maps [B, ...] of one shape, flattened per sample -> (scale, shift),
    [B,1,1,1] each in mde's dtype."""
    for t, name in ((mde, "mde"), (disp, "disp"), (conf, "conf")):
        _on_gpu(t, name)
        if t.dim() < 2 or t.shape != mde.shape:
            raise RuntimeError(f"weighted_lsq: {name} must be [B, ...] of mde's shape {tuple(mde.shape)}, "
                               f"got {tuple(t.shape)}")
    B = mde.shape[0]
    m, d, c = (t.reshape(B, -1).float().contiguous() for t in (mde, disp, conf))
    if _wants_grad(m, d, c):
        scale, shift = _WeightedLsqFn.apply(m, d, c, float(min_quantile), float(max_quantile))
    else:
        scale, shift = ops.weighted_lsq(m, d, c, float(min_quantile), float(max_quantile))
    return scale.reshape(B, 1, 1, 1).to(mde.dtype), shift.reshape(B, 1, 1, 1).to(mde.dtype)


# ------------------------------------------------------------------------------- volume stage
class VolumeCorruption(NamedTuple):
    """One drawn volume-corruption augmentation (stereoanywhere.py:217-251): which volume, which
    branch, the depth bin of the left mono map it acts in and, for a roll, the shift along W1."""
    target: str   # "stereo" | "mono"
    kind: str     # "roll" | "noise" | "zero"
    bin: int
    shift: int    # 1..w_lowres for a roll, else 0


_BRANCHES = tuple((t, k) for t in ("stereo", "mono") for k in ("roll", "noise", "zero"))


def draw_volume_corruption(prob: float, n_masks: int, w_lowres: int, rng=random) -> Optional[VolumeCorruption]:
    """The reference's draws at stereoanywhere.py:218-251 in their order: one ``rng.random()`` per
    branch until one fires (``< prob``), then ``rng.randint(0, n_masks - 1)`` for the bin and, for a
    roll, ``rng.randint(1, w_lowres)`` for the shift.  None when no branch fires (six draws).  rng: the
    ``random`` module or a ``random.Random``; seeded like the reference's it gives the reference's plan."""
    for target, kind in _BRANCHES:
        if rng.random() < prob:
            bin_ = rng.randint(0, n_masks - 1)
            shift = rng.randint(1, w_lowres) if kind == "roll" else 0
            return VolumeCorruption(target, kind, bin_, shift)
    return None


def _stage_volume(v: torch.Tensor, name: str) -> torch.Tensor:
    _on_gpu(v, name)
    if v.dim() != 5 or v.shape[1] != 1:
        raise RuntimeError(f"{name} must be [B,1,H,W1,W2], got {tuple(v.shape)}")
    return v.float().contiguous()


def _stage_map(t: torch.Tensor, name: str, vol: torch.Tensor) -> torch.Tensor:
    """A per-left-pixel map of the volume: [B,1,H,W1] (or [B,1,H,W1,1], the reference's unsqueezed form)."""
    _on_gpu(t, name)
    B, _, H, W1, _ = vol.shape
    if tuple(t.shape) not in ((B, 1, H, W1), (B, 1, H, W1, 1)):
        raise RuntimeError(f"{name} must be [B,1,H,W1] = {(B, 1, H, W1)} for a volume {tuple(vol.shape)}, "
                           f"got {tuple(t.shape)}")
    return t.detach().float().contiguous()


def _check_plan(plan: VolumeCorruption, n_masks: int, vol: torch.Tensor) -> None:
    if plan.kind not in ("roll", "noise", "zero"):
        raise RuntimeError(f"volume corruption kind must be 'roll', 'noise' or 'zero', got {plan.kind!r}")
    if plan.target not in ("stereo", "mono"):
        raise RuntimeError(f"volume corruption target must be 'stereo' or 'mono', got {plan.target!r}")
    if not 0 <= plan.bin < n_masks:
        raise RuntimeError(f"volume corruption bin must be 0..{n_masks - 1}, got {plan.bin}")
    if plan.kind == "roll" and not 1 <= plan.shift <= vol.shape[3]:
        raise RuntimeError(f"volume corruption shift must be 1..W1 = {vol.shape[3]}, got {plan.shift}")
    if plan.kind == "zero" and vol.shape[3] != vol.shape[4]:
        raise RuntimeError(f"the 'zero' corruption needs W1 == W2, got a volume {tuple(vol.shape)}")


def _truncation(truncate, vol: torch.Tensor):
    disp, conf, atten = truncate
    if vol.shape[3] != vol.shape[4]:
        raise RuntimeError(f"the truncation needs W1 == W2, got a volume {tuple(vol.shape)}")
    return _stage_map(disp, "disp_left", vol), _stage_map(conf, "conf_left", vol), float(atten)


def _stage_launch(vol, mde, plan, noise, n_masks, trunc):
    """One sa_volume_stage launch (plus sa_volume_peak's two for "zero") -> a new tensor."""
    kw = {}
    if plan is not None:
        _check_plan(plan, n_masks, vol)
        if mde is None:
            raise RuntimeError("a volume corruption needs mde_lowres [B,1,H,W1]")
        kw = dict(kind=plan.kind, mde=_stage_map(mde, "mde_lowres", vol), nbins=n_masks, bin=plan.bin,
                  shift=plan.shift if plan.kind == "roll" else 1)
        if plan.kind == "noise":
            if noise is None:   # the reference's rand_like of its fp16 mask: the same generator draws
                B, _, H, W1, _ = vol.shape
                noise = torch.rand((B, 1, H, W1, 1), dtype=torch.float16, device=vol.device)
            kw["noise"] = _stage_map(noise, "noise", vol)
        elif plan.kind == "zero":
            kw["peak"] = ops.volume_peak(vol)
    if trunc is not None:
        kw.update(trunc_disp=trunc[0], trunc_conf=trunc[1], atten=trunc[2])
    return ops.volume_stage(vol, **kw)


def corrupt_volume(volume, mde_lowres, plan: VolumeCorruption, noise=None, n_masks: int = 4) -> torch.Tensor:
    """One branch of the reference's volume-corruption augmentations (stereoanywhere.py:217-251) on
    volume [B,1,H,W1,W2]: inside depth bin ``plan.bin`` of ``n_masks`` (``vol_aug_n_masks``) of the left
    mono map mde_lowres [B,1,H,W1] the volume is rolled by ``plan.shift`` along W1, multiplied by a
    per-pixel noise, or multiplied by max(volume) * exp(-(j - k)^2 / 2); elsewhere it is copied.  One
    launch (three for "zero": the maximum stays on the device).  Returns a new, detached fp32 tensor,
    as the reference detaches these results.  noise ("noise" only): [B,1,H,W1,1] fp16 or fp32; None
    draws ``torch.rand(..., dtype=float16)``, the reference's ``rand_like`` of its fp16 mask."""
    vol = _stage_volume(volume, "volume").detach()
    if plan is None:
        raise RuntimeError("corrupt_volume: plan is None (draw_volume_corruption drew no branch)")
    return _stage_launch(vol, mde_lowres, plan, noise, n_masks, None)


class _TruncateFn(torch.autograd.Function):
    """ops.volume_stage's truncation with ops.volume_truncate_backward as its adjoint.  Saves the two
    maps; the factor is recomputed.  The maps get no gradient (the reference detaches the mask)."""

    @staticmethod
    def forward(ctx, volume, disp, conf, atten):
        ctx.save_for_backward(disp, conf)
        ctx.atten = atten
        return ops.volume_stage(volume, trunc_disp=disp, trunc_conf=conf, atten=atten)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        disp, conf = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        return ops.volume_truncate_backward(grad.float().contiguous(), disp, conf, ctx.atten), None, None, None


def truncate_volume(volume, disp_left, conf_left, attenuation_gain: float = 0.9) -> torch.Tensor:
    """``truncate_corr_volume_v2(disp_left, conf_left, conf_th=None, attenuation_gain).detach() * volume``
    (stereoanywhere.py:203, 253-254) in one launch: volume [B,1,H,W,W], maps [B,1,H,W].  Differentiable
    with respect to the volume only."""
    vol = _stage_volume(volume, "volume")
    disp, conf, atten = _truncation((disp_left, conf_left, attenuation_gain), vol)
    if _wants_grad(vol):
        return _TruncateFn.apply(vol, disp, conf, atten)
    return ops.volume_stage(vol, trunc_disp=disp, trunc_conf=conf, atten=atten)


def volume_stage(stereo, mono, mde_lowres=None, plan: Optional[VolumeCorruption] = None, truncate=None, noise=None,
                 n_masks: int = 4):
    """What stands between the aggregated volumes and the two ``corr_block(...)`` constructors
    (stereoanywhere.py:214-255) -> (stereo_out, mono_out).  plan: ``draw_volume_corruption``'s result;
    truncate: (disp_left, conf_left, attenuation_gain) or None (``use_truncate_vol`` off).  A corrupted
    stereo volume gets its corruption and its truncation in one launch and is detached; an uncorrupted
    one goes through ``truncate_volume`` and keeps its ``grad_fn``.  A volume nothing touches is
    returned as the same tensor."""
    if plan is not None and plan.target == "mono":
        mono = corrupt_volume(mono, mde_lowres, plan, noise, n_masks)
        plan = None
    if plan is not None:
        vol = _stage_volume(stereo, "stereo").detach()
        trunc = None if truncate is None else _truncation(truncate, vol)
        stereo = _stage_launch(vol, mde_lowres, plan, noise, n_masks, trunc)
    elif truncate is not None:
        stereo = truncate_volume(stereo, *truncate)
    return stereo, mono


# ------------------------------------------------------------------------------- volume close
class _VolumeCloseFn(torch.autograd.Function):
    """ops.volume_close_stats + ops.vol_apply with ops.volume_close_backward as the adjoint.  Saves x, the
    two gate maps and mean / rstd; the normalised, activated and gated volumes are recomputed."""

    @staticmethod
    def forward(ctx, x, gate_left, gate_right, slope, eps):
        mean, rstd = ops.volume_close_stats(x, eps)
        ctx.save_for_backward(x, gate_left, gate_right, mean, rstd)
        ctx.slope = slope
        gate = None if gate_left is None else (gate_left, gate_right)
        return ops.vol_apply(ops.VolAct(x, (mean, rstd), act=True, gate=gate), slope).raw

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        x, gate_left, gate_right, mean, rstd = ctx.saved_tensors
        need_x, need_l, need_r = ctx.needs_input_grad[:3]
        if not (need_x or need_l or need_r):
            return None, None, None, None, None
        dx, dgl, dgr = ops.volume_close_backward(grad.float().contiguous(), x, mean, rstd, gate_left, gate_right,
                                                 ctx.slope, need_x, need_l, need_r)
        return dx, dgl, dgr, None, None


def _close_map(t: torch.Tensor, name: str, shape) -> torch.Tensor:
    _on_gpu(t, name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"volume_close: {name} must be {tuple(shape)} for this volume, got {tuple(t.shape)}")
    return t.float().contiguous()


def volume_close(x, gate_left=None, gate_right=None, negative_slope: float = 0.01, eps: float = 1e-5) -> torch.Tensor:
    """``gate * leaky_relu(instance_norm(x), negative_slope)``: the close of an hourglass layer
    (submodule.py:25-53, 113-140) on a volume x [B,C,D,H,W] that any conv produced, as three streaming
    HIP passes forward and five backward (csrc/volume_close.hip).  gate_left [B,C,H,W] and gate_right
    [B,C,H,D] are the sigmoid'ed DoubleFeatureAtt maps at the volume's own resolution (both or neither);
    the gate is ``gate_left[:, :, None] * gate_right.permute(0, 1, 3, 2)[..., None]``.  Differentiable
    with respect to x and both maps (the sigmoid stays with the caller, so autograd carries the map
    gradients on).  Instance statistics (biased variance, ``affine=False``) in every mode."""
    _on_gpu(x, "x")
    if x.dim() != 5:
        raise ValueError(f"volume_close: x must be [B,C,D,H,W], got {tuple(x.shape)}")
    if (gate_left is None) != (gate_right is None):
        raise ValueError("volume_close: give both gate maps or neither")
    B, C, D, H, W = x.shape
    if D * H * W <= 1:
        raise ValueError(f"volume_close: instance norm needs more than one cell per channel, got {tuple(x.shape)}")
    x = x.float().contiguous()
    if gate_left is not None:
        gate_left = _close_map(gate_left, "gate_left", (B, C, H, W))
        gate_right = _close_map(gate_right, "gate_right", (B, C, H, D))
    return _VolumeCloseFn.apply(x, gate_left, gate_right, float(negative_slope), float(eps))


# ------------------------------------------------------------------------------- up-cat conv
# (skip channels, low-branch channels, output channels) of the hourglass's two joins (hourglass.py:319-321,
# 326-328): what sa_conv3d_pointwise, sa_conv3d_pointwise_upcat and sa_conv3d_pointwise_backward are built for
UPCAT_TRIPLES = ((8, 16, 8), (16, 32, 16))
# ((Ca, Cu, Cout), low_first) of the published 8-channel hourglass: final_agg[0] over cat(orig, up) and
# agg_layers[1][0] over cat(up, down0); hourglass_forward(joins="hip") takes upcat_conv for these
HOURGLASS_JOINS = (((8, 16, 8), False), ((16, 32, 16), True))


def _upcat_problem(skip, low, weight):
    """None when ``upcat_conv`` is built for these tensors, else what is wrong with them."""
    if skip.dim() != 5 or low.dim() != 5 or weight.dim() != 5:
        return f"skip, low and weight must be 5-D, got {tuple(skip.shape)}, {tuple(low.shape)}, {tuple(weight.shape)}"
    (B, ca, D, H, W), (Bl, cu, Dp, Hp, Wp) = skip.shape, low.shape
    cout = weight.shape[0]
    if tuple(weight.shape[1:]) != (ca + cu, 1, 1, 1) or Bl != B:
        return (f"weight must be [Cout, Ca + Cu = {ca + cu}, 1, 1, 1] and the batches equal, got weight "
                f"{tuple(weight.shape)}, skip {tuple(skip.shape)}, low {tuple(low.shape)}")
    if (ca, cu, cout) not in UPCAT_TRIPLES:
        return f"built for (Ca, Cu, Cout) in {UPCAT_TRIPLES}, got {(ca, cu, cout)}"
    if min(D, H, W) < 2:
        return f"D, H and W must be at least 2, got {(D, H, W)}"
    if min(Dp, Hp, Wp) < 1 or any(2 * (n - 1) > N - 1 for n, N in zip((Dp, Hp, Wp), (D, H, W))):
        return (f"the low branch must be at most half size (2 (n - 1) <= N - 1 per axis), got {(Dp, Hp, Wp)} "
                f"under {(D, H, W)}")
    if D * H * W >= 2 ** 31:
        return f"D*H*W must be below 2^31, got {(D, H, W)}"
    return None


def _upcat_weights(weight, ca: int, low_first: bool):
    """The module's [Cout, Ca+Cu, 1, 1, 1] weight -> (w_a [Ca][Cout], w_u [Cu][Cout]), contiguous."""
    w = weight.reshape(weight.shape[0], -1)
    cu = w.shape[1] - ca
    w_a, w_u = (w[:, cu:], w[:, :cu]) if low_first else (w[:, :ca], w[:, ca:])
    return w_a.t().contiguous(), w_u.t().contiguous()


class _UpcatConvFn(torch.autograd.Function):
    """ops.conv3d_pointwise_upcat (Wa . skip + up(Wu . low), two launches) with ops.trilinear_up_adjoint and
    ops.conv3d_pointwise_backward as the adjoint.  Saves skip, low and the weight: the up-sampled and the
    concatenated volume exist in neither direction."""

    @staticmethod
    def forward(ctx, skip, low, weight, low_first):
        ctx.save_for_backward(skip, low, weight)
        ctx.low_first = low_first
        w_a, w_u = _upcat_weights(weight, skip.shape[1], low_first)
        return ops.conv3d_pointwise_upcat(ops.VolAct(skip), ops.VolAct(low), w_a, w_u, weight.shape[0],
                                          stats=False).raw

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        skip, low, weight = ctx.saved_tensors
        need_skip, need_low, need_w = ctx.needs_input_grad[:3]
        if not (need_skip or need_low or need_w):
            return None, None, None, None
        grad = grad.float().contiguous()
        w_a, w_u = _upcat_weights(weight, skip.shape[1], ctx.low_first)
        d_skip = d_low = d_weight = dw_a = dw_u = None
        if need_skip or need_w:
            d_skip, dw_a = ops.conv3d_pointwise_backward(skip, grad, w_a, need_skip, need_w)
        if need_low or need_w:
            dp = ops.trilinear_up_adjoint(grad, low.shape[2:])
            d_low, dw_u = ops.conv3d_pointwise_backward(low, dp, w_u, need_low, need_w)
        if need_w:
            d_weight = torch.cat((dw_u, dw_a) if ctx.low_first else (dw_a, dw_u), 0).t().reshape(weight.shape)
        return d_skip, d_low, d_weight, None


def upcat_conv(skip, low, weight, low_first: bool) -> torch.Tensor:
    """``conv3d(cat((up(low), skip) if low_first else (skip, up(low)), 1), weight)`` with
    ``up = interpolate(size=skip.shape[2:], mode="trilinear", align_corners=True)``: a join of the hourglass
    (hourglass.py:319-321, 326-328) as ``Wa . skip + up(Wu . low)``, the low branch projected onto the output
    channels before it is up-sampled, so neither the up-sampled nor the concatenated volume is written or
    kept (csrc/conv3d_fused.hip forward, csrc/upcat_backward.hip backward).  skip [B,Ca,D,H,W], low
    [B,Cu,Dp,Hp,Wp] at most half size per axis, weight the module's own [Cout, Ca+Cu, 1, 1, 1] (no bias);
    built for (Ca, Cu, Cout) in ``UPCAT_TRIPLES``.  Differentiable with respect to all three; saves exactly
    them; each gradient is computed only where it is needed."""
    for t, name in ((skip, "skip"), (low, "low"), (weight, "weight")):
        _on_gpu(t, name)
    problem = _upcat_problem(skip, low, weight)
    if problem is not None:
        raise ValueError(f"upcat_conv: {problem}")
    return _UpcatConvFn.apply(skip.float().contiguous(), low.float().contiguous(), weight.float().contiguous(),
                              bool(low_first))


def _join(conv, skip, low, low_first: bool, joins: str):
    """The first conv of a join's Sequential on cat(skip, up(low)): ``upcat_conv`` with joins="hip" where the
    join is one of the published hourglass's two (``HOURGLASS_JOINS``) on a plain 1x1x1 conv and the sizes
    are built, else torch's interpolate + cat + conv: a narrower or wider hourglass runs wholly on torch."""
    triple = (skip.shape[1], low.shape[1], getattr(conv, "out_channels", None))
    if (joins == "hip" and (triple, low_first) in HOURGLASS_JOINS and isinstance(conv, torch.nn.Conv3d)
            and conv.bias is None and conv.groups == 1
            and tuple(conv.stride) == (1, 1, 1) and tuple(conv.padding) == (0, 0, 0)
            and _upcat_problem(skip, low, conv.weight) is None):
        return upcat_conv(skip, low, conv.weight, low_first)
    up = torch.nn.functional.interpolate(low, size=skip.shape[2:], mode="trilinear", align_corners=True)
    return conv(torch.cat((up, skip) if low_first else (skip, up), 1))


# ------------------------------------------------------------------------------- 3x3x3 conv
def _k3_problem(x, weight):
    """None when ``conv3d_k3`` is built for these tensors, else what is wrong with them."""
    if x.dim() != 5 or weight.dim() != 5:
        return f"x and weight must be 5-D, got {tuple(x.shape)}, {tuple(weight.shape)}"
    B, C, D, H, W = x.shape
    if C not in ops.CONV3D_K3_CHANNELS or tuple(weight.shape) != (C, C, 3, 3, 3):
        return (f"built for [C, C, 3, 3, 3] weights with C in {ops.CONV3D_K3_CHANNELS} on [B, C, D, H, W], got "
                f"weight {tuple(weight.shape)}, x {tuple(x.shape)}")
    if min(B, D, H, W) < 1:
        return f"empty volume {tuple(x.shape)}"
    if D * H * W >= 2 ** 30:
        return f"D*H*W must be below 2^30, got {(D, H, W)}"
    if C * D * H * W * 4 >= 2 ** 31:
        return f"a sample's volume C*D*H*W*4 must be below 2^31 bytes, got {(C, D, H, W)}"
    return None


class _Conv3dK3Fn(torch.autograd.Function):
    """sa_conv3d_mf_scaled forward and, on the flipped and channel-swapped table, for dx;
    sa_conv3d_k3_backward_weight for dw.  Saves x and the weight; both tables and every scale are rebuilt."""

    @staticmethod
    def forward(ctx, x, weight, x_bounded):
        ctx.save_for_backward(x, weight)
        ctx.x_bounded = x_bounded
        C = x.shape[1]
        table = ops.conv3d_mf_table(weight.reshape(C, C, 27).permute(1, 2, 0).contiguous())   # [ci][tap][co]
        scales = (None, None) if x_bounded else ops.sample_scale(x, C)
        return ops.conv3d_mf_scaled(x, table, *scales)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        x, weight = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[:2]
        if not (need_x or need_w):
            return None, None, None
        grad = grad.float().contiguous()
        B, C = x.shape[:2]
        g_scale, g_inv = ops.sample_scale(grad, C)   # one launch, for dx and dw
        dx = dw = None
        if need_x:
            # dx[ci] = sum_co conv(g[co], w[co][ci] flipped): a conv with co as its input channels
            table = ops.conv3d_mf_table(weight.reshape(C, C, 27).flip(2).permute(0, 2, 1).contiguous())
            dx = ops.conv3d_mf_scaled(grad, table, g_scale, g_inv)
        if need_w:
            x_scale = None if ctx.x_bounded else ops.sample_scale(x, 1)[0]
            dw_t = ops.conv3d_k3_backward_weight(x, grad, x_scale, g_scale.view(B, C)[:, 0].contiguous())
            dw = dw_t.permute(2, 0, 1).reshape(weight.shape)
        return dx, dw, None


def conv3d_k3(x, weight, x_bounded: bool = False, check_weight: bool = False) -> torch.Tensor:
    """``F.conv3d(x, weight, padding=1)`` for x [B,C,D,H,W] and the module's own [C, C, 3, 3, 3] weight (stride
    1, no bias), C in ``ops.CONV3D_K3_CHANNELS``, on the inference path's split-f16 MFMA kernel at fp32-level
    accuracy (csrc/conv3d_mfma.hip), differentiable with respect to both (csrc/conv3d_backward.hip): dx is the
    same kernel on the gradient with the flipped, channel-swapped weight, dw a split-f16 MFMA reduction over
    cells folded in float64.  Saves exactly x and weight; each gradient is computed only where it is needed.

    The kernel needs |value| < 2^15.  A gradient has no such bound, so it is multiplied per sample by a power
    of two that brings its maximum into [2^13, 2^14) and the result divided by it again (exact; found on the
    device, no host sync); x is treated the same way unless ``x_bounded`` declares |x| < 2^15, which holds
    for every InstanceNorm'ed volume.  A value below 2^-27 of its sample's maximum loses relative precision.

    No call reads anything back to the host.  That includes the weight's range: the inference path's
    |w| < 8 is not checked, and a weight whose 2^12-fold leaves f16's range (|w| >= 15.996) gives non-finite
    outputs (its split halves are inf and -inf), which a loss's NaN rules catch.  ``check_weight=True`` runs
    the blocking |w| < 8 check and raises instead; for debugging."""
    for t, name in ((x, "x"), (weight, "weight")):
        _on_gpu(t, name)
    problem = _k3_problem(x, weight)
    if problem is not None:
        raise ValueError(f"conv3d_k3: {problem}")
    if check_weight and not bool((weight.detach().abs() < 8.0).all()):
        raise ValueError("conv3d_k3: a weight is outside the split range |w| < 8")
    return _Conv3dK3Fn.apply(x.float().contiguous(), weight.float().contiguous(), bool(x_bounded))


def _conv(conv, x, convs: str):
    """A BasicConv's own conv: ``conv3d_k3`` with convs="hip" where it is a plain stride-1, pad-1 3x3x3
    nn.Conv3d with equal channel counts that the kernel is built for (its input is a ``volume_close`` output,
    so |x| <= sqrt(cells) < 2^15), else the module on torch."""
    if (convs == "hip" and isinstance(conv, torch.nn.Conv3d) and conv.bias is None and conv.groups == 1
            and tuple(conv.kernel_size) == (3, 3, 3) and tuple(conv.stride) == (1, 1, 1)
            and tuple(conv.padding) == (1, 1, 1) and tuple(conv.dilation) == (1, 1, 1)
            and conv.padding_mode == "zeros" and conv.in_channels == conv.out_channels
            and x.is_cuda and _k3_problem(x, conv.weight) is None):
        return conv3d_k3(x, conv.weight, x_bounded=True)
    return conv(x)


def _close_layer(conv_block, x, gate=None, conv_out=None, convs: str = "torch"):
    """One BasicConv (its own nn.Conv3d unless its output ``conv_out`` is given, then the fused close) -> its
    output volume."""
    return volume_close(_conv(conv_block.conv, x, convs) if conv_out is None else conv_out, *(gate or (None, None)),
                        negative_slope=getattr(conv_block.act_fn, "negative_slope", 0.01),
                        eps=getattr(conv_block.norm_fn, "eps", 1e-5))


def _close_gated(layers, att, x, feat_left, feat_right, first=None, convs: str = "torch"):
    """A Sequential of BasicConvs followed by a DoubleFeatureAtt: the gate goes into the last close when
    its maps are at the volume's resolution, else that close runs gate-less and the module's own
    interpolate-and-multiply follows.  ``first``: the first layer's conv output where a join made it
    (x is unused then)."""
    for k, layer in enumerate(list(layers)[:-1]):
        # (a Sequential's first conv reads the caller's x, whose range nobody vouches for: on torch)
        x = _close_layer(layer, x, conv_out=first if k == 0 else None, convs=convs if k > 0 else "torch")
    y = first if first is not None and len(layers) == 1 else _conv(layers[-1].conv, x, convs if len(layers) > 1 else "torch")
    gl = torch.sigmoid(att.feat_att_left(feat_left))
    gr = torch.sigmoid(att.feat_att_right(feat_right))
    D, H, W = y.shape[2:]
    last = dict(negative_slope=getattr(layers[-1].act_fn, "negative_slope", 0.01),
                eps=getattr(layers[-1].norm_fn, "eps", 1e-5))
    if tuple(gl.shape[2:]) == (H, W) and tuple(gr.shape[2:]) == (H, D):
        return volume_close(y, gl, gr, **last)
    g = gl.unsqueeze(2) * gr.permute(0, 1, 3, 2).unsqueeze(4)
    g = torch.nn.functional.interpolate(g, size=(D, H, W), mode="trilinear", align_corners=True)
    return g * volume_close(y, **last)


def hourglass_forward(hg, x, features_left, features_right, layout: str = "reference", joins: str = "torch",
                      convs: str = "torch"):
    """The live part of the reference's ``Hourglass.forward`` (hourglass.py:61-91) for fine-tuning: the
    module's own ``nn.Conv3d``s on torch / MIOpen, every InstanceNorm3d + LeakyReLU (+ the following
    DoubleFeatureAtt) as one ``volume_close``.  The deepest down layer and the first up-path step feed
    nothing (``blocks.Hourglass``'s docstring) and are skipped, so their parameters get no gradient.

    ``hg``: the reference's ``Hourglass`` or ``blocks.Hourglass`` (only ``down_layers``, ``agg_layers``,
    ``final_agg``, ``feature_atts``, ``feature_atts_up``, ``final_feature_atts_up`` and
    ``number_of_scales`` are used).  layout="reference" takes and returns [B,C,H,W1,W2] with the
    reference's permutes (``types.MethodType(hourglass_forward, hg)`` replaces its forward);
    layout="volume" works on [B,C,W2,H,W1].  joins="torch": the two joins (trilinear up-sampling, ``cat``
    and the 1x1x1 conv) stay on torch; joins="hip": each runs as one ``upcat_conv`` where that is built
    for its channels and sizes (the published 8-channel hourglass), else on torch.  convs="torch": every
    ``nn.Conv3d`` on torch; convs="hip": each stride-1 3x3x3 conv with equal channel counts that follows a close
    (six of the published hourglass's eight) runs as ``conv3d_k3(..., x_bounded=True)`` where that is built for
    its channels and sizes, else on torch; the stride-2 convs stay on torch."""
    if layout not in ("reference", "volume"):
        raise ValueError(f"hourglass_forward: layout must be 'reference' or 'volume', got {layout!r}")
    if joins not in ("torch", "hip"):
        raise ValueError(f"hourglass_forward: joins must be 'torch' or 'hip', got {joins!r}")
    if convs not in ("torch", "hip"):
        raise ValueError(f"hourglass_forward: convs must be 'torch' or 'hip', got {convs!r}")
    ns = hg.number_of_scales
    if layout == "reference":
        x = x.permute(0, 1, 3, 2, 4).permute(0, 1, 4, 3, 2)
    orig = x
    downs = []
    for i in range(ns - 2):
        x = _close_gated(hg.down_layers[i], hg.feature_atts[i], x, features_left[i + 1], features_right[i + 1],
                         convs=convs)
        downs.append(x)
    i = ns - 3
    y = _join(hg.agg_layers[i][0].conv, downs[ns - 3 - i], downs[ns - 2 - i], True, joins)
    x = _close_gated(hg.agg_layers[i], hg.feature_atts_up[i], None, features_left[ns - 2 - i],
                     features_right[ns - 2 - i], first=y, convs=convs)
    y = _join(hg.final_agg[0].conv, orig, x, False, joins)
    x = _close_gated(hg.final_agg, hg.final_feature_atts_up, None, features_left[0], features_right[0], first=y,
                     convs=convs)
    if layout == "reference":
        x = x.permute(0, 1, 4, 3, 2).permute(0, 1, 3, 2, 4)
    return x

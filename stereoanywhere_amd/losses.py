"""The reference's training loss (train.py:281-379) as one fused, differentiable HIP op.

``sequence_loss`` is the iterative-prediction block (train.py:290-316), ``coarse_loss`` the coarse
block of one side (321-344 left, 350-377 right), ``training_loss`` the whole of it from the six-tuple
of ``forward(test_mode=False)``; ``loss_terms`` is the op underneath for any list of maps.  The
formulas, the NaN rules (which terms train.py drops and which it lets propagate) and the arithmetic
are written down once, in include/stereoanywhere_hip.h ("The fused training loss").

With grad mode on and a map or confidence that requires grad the op runs as an autograd function:
the forward is ``ops.loss_terms`` (three launches per 32 maps), the backward ``ops.loss_terms_backward``
(one launch per 32 maps), deterministic, recomputing from the inputs; it saves its inputs and a record
of a few doubles per map (the counts, which terms were dropped, min / max per sample), nothing
plane-sized.  Otherwise it makes the plain ``ops`` call and returns tensors without a ``grad_fn``.
Neither direction synchronises with the host: the NaN checks of train.py happen on the device.  Double
backward is not built.

Inputs are fp32 GPU tensors [B,1,H,W]; anything else is refused (there is no CPU path; cast
fp16 / bf16 activations with ``.float()``, which autograd carries back).  Ground truth, validity and
the mono maps carry no gradient.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .corr import _wants_grad
from .ops import LossMap

__all__ = ["LossMap", "loss_terms", "sequence_loss", "coarse_loss", "training_loss"]


def _map(t, name: str, like: Optional[torch.Tensor] = None, channels: int = 1) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} must be on the GPU (the HIP loss has no CPU fallback), got {t.device}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (cast with .float()), got {t.dtype}")
    if t.dim() != 4 or t.shape[1] != channels:
        raise RuntimeError(f"{name} must be [B,{channels},H,W], got {tuple(t.shape)}")
    if like is not None and (t.shape[0], t.shape[2], t.shape[3]) != (like.shape[0], like.shape[2], like.shape[3]):
        raise RuntimeError(f"{name} must be [B,{channels},H,W] with gt's B, H, W {tuple(like.shape)}, "
                           f"got {tuple(t.shape)}")
    return t.contiguous()


class _LossTermsFn(torch.autograd.Function):
    """ops.loss_terms with ops.loss_terms_backward as its adjoint over a variable number of maps and
    confidences.  Saves its inputs and the forward's record."""

    @staticmethod
    def forward(ctx, consts, scalars, gt, valid, target, *tensors):
        maps = _assemble(consts, tensors)
        out, rec = ops.loss_terms(maps, gt, valid, target=target, **scalars)
        ctx.save_for_backward(gt, valid, target, rec, *tensors)
        ctx.consts, ctx.scalars = consts, scalars
        ctx.mark_non_differentiable(out)
        return rec[0].clone(), out   # the total before its rounding to fp32

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, _g_terms):
        gt, valid, target, rec, *tensors = ctx.saved_tensors
        need = ctx.needs_input_grad[5:]
        if g_total is None or not any(need):
            return (None,) * (5 + len(tensors))
        maps = _assemble(ctx.consts, tensors)
        K = len(maps)
        need_map = list(need[:K])
        it = iter(need[K:])
        need_conf = [M.conf is not None and next(it) for M in maps]
        s = ctx.scalars
        g_maps, g_confs = ops.loss_terms_backward(maps, gt, valid, s["maxdisp"], target, s["gain"], s["border"],
                                                  s["lrc_th"], rec, g_total.float().reshape(1).contiguous(),
                                                  need_map, need_conf)
        return (None, None, None, None, None, *g_maps, *[g for g, M in zip(g_confs, maps) if M.conf is not None])


def _assemble(consts, tensors):
    """LossMaps from the per-map constants (has_conf, sign, sel, w_l1, w_n, w_bce, flags) and the flat
    tensor list (the K maps, then the confidences of the maps that have one)."""
    K = len(consts)
    confs = iter(tensors[K:])
    return [LossMap(tensors[k], next(confs) if c[0] else None, *c[1:]) for k, c in enumerate(consts)]


def loss_terms(maps: Sequence[LossMap], gt, valid, *, maxdisp: float, target=None, gain: float = 1.0,
               border: str = "none", lrc_th: float = 1.0, _fp64: bool = False):
    """The fused loss of any list of maps -> (total, terms [K,3]): the differentiable scalar and the
    detached L1_k, N_k, BCE_k (0 where a term is not computed or its map was skipped).  (_fp64: the
    total as the float64 it was added up in, for training_loss to add three of them and round once.)"""
    gt = _map(gt, "gt")
    valid = _map(valid, "valid", gt)
    if target is not None:
        target = _map(target, "target", gt, 3)
    maps = [M._replace(map=_map(M.map, f"map {k}", gt), conf=None if M.conf is None else _map(M.conf, f"conf {k}", gt))
            for k, M in enumerate(maps)]
    if not maps:
        raise ValueError("loss_terms: at least one map is needed")
    for k, M in enumerate(maps):
        if M.sign not in (-1, 1):
            raise ValueError(f"loss_terms: map {k}: sign must be -1 or +1, got {M.sign}")
    scalars = dict(maxdisp=float(maxdisp), gain=float(gain), border=border, lrc_th=float(lrc_th))
    tensors = [M.map for M in maps] + [M.conf for M in maps if M.conf is not None]
    if _wants_grad(*tensors):
        consts = tuple((M.conf is not None, int(M.sign), int(M.sel), float(M.w_l1), float(M.w_n), float(M.w_bce),
                        int(M.flags)) for M in maps)
        total, out = _LossTermsFn.apply(consts, scalars, gt, valid, target, *tensors)
    else:
        out, rec = ops.loss_terms(maps, gt, valid, target=target, **scalars)
        total = rec[0].clone()
    return (total if _fp64 else total.float()), out[1:].reshape(len(maps), 3)


def _target(mono, gt: torch.Tensor, normal_gain: float, who: str):
    """estimate_normals(mono, W / normal_gain) (train.py:287-288), without gradient."""
    if mono is None:
        raise ValueError(f"{who}: the normals loss needs the mono map")
    with torch.no_grad():
        return ops.mono_normals(_map(mono, "mono", gt), gt.shape[-1] / normal_gain)


def _sequence_maps(pred_disps, pred_confs, loss_gamma: float, use_normal_loss: bool):
    n = len(pred_disps)
    if n < 2:
        raise ValueError(f"sequence_loss: at least 2 predictions are needed, got {n} (the weights are "
                         "loss_gamma ** (15 / (n - 1)) powers: train.py:295 divides by zero)")
    if pred_confs is not None and len(pred_confs) != n:
        raise ValueError(f"sequence_loss: {len(pred_confs)} confidences for {n} predictions")
    maps = []
    for i, p in enumerate(pred_disps):
        w = (loss_gamma ** (15 / (n - 1))) ** (n - i - 1)
        c = None if pred_confs is None else pred_confs[i]
        maps.append(LossMap(p, c, -1, ops.LOSS_SEL_MASK, w, 10 * w if use_normal_loss else 0.0,
                            w if c is not None else 0.0, ops.LOSS_DROP_NAN_BCE))
    return maps


def _sequence(pred_disps, gt, valid, *, maxdisp, mono=None, normal_gain=10, use_normal_loss=False, loss_gamma=0.9,
              pred_confs=None, lrc_th=1.0, target=None, _fp64=False):
    maps = _sequence_maps(pred_disps, pred_confs, loss_gamma, use_normal_loss)
    if use_normal_loss and target is None:
        target = _target(mono, _map(gt, "gt"), normal_gain, "sequence_loss")
    return loss_terms(maps, gt, valid, maxdisp=maxdisp, target=target if use_normal_loss else None,
                      gain=gt.shape[-1] / normal_gain, border="none", lrc_th=lrc_th, _fp64=_fp64)


def sequence_loss(pred_disps, gt, valid, *, maxdisp, mono=None, normal_gain=10, use_normal_loss=False,
                  loss_gamma=0.9, pred_confs=None, lrc_th=1.0):
    """train.py:290-316 -> the scalar: the predictions are -disparity (sign -1); per prediction
    i_weight = (loss_gamma ** (15 / (n - 1))) ** (n - i - 1) times the L1 over mask, 10 i_weight times
    the normals term against estimate_normals(mono, W / normal_gain) (NaN: dropped), and where
    ``pred_confs[i]`` is given i_weight times its BCE (NaN: dropped).  A NaN L1 propagates."""
    return _sequence(pred_disps, gt, valid, maxdisp=maxdisp, mono=mono, normal_gain=normal_gain,
                     use_normal_loss=use_normal_loss, loss_gamma=loss_gamma, pred_confs=pred_confs, lrc_th=lrc_th)[0]


def _coarse(disps, confs, gt, valid, *, maxdisp, side, mono=None, normal_gain=10, use_normal_loss_on_coarse=False,
            use_border_mask=False, lrc_th=1.0, target=None, _fp64=False):
    if side not in ("left", "right"):
        raise ValueError(f"coarse_loss: side must be 'left' or 'right', got {side!r}")
    if len(disps) != 3 or len(confs) != 3:
        raise ValueError(f"coarse_loss: three disparities and three confidences (None to skip one) are expected, "
                         f"got {len(disps)} and {len(confs)}")
    maps = []
    for i, (d, c) in enumerate(zip(disps, confs)):
        if d is None:
            continue
        flags = ops.LOSS_SKIP_IF_NAN_MAP | ops.LOSS_DROP_NAN_L1 | (ops.LOSS_DROP_NAN_BCE if side == "right" else 0)
        maps.append(LossMap(d, c, 1, ops.LOSS_SEL_MASK if i == 2 else ops.LOSS_SEL_MASK_BORDER, 1.0,
                            10.0 if (use_normal_loss_on_coarse and i != 2) else 0.0, 1.0 if c is not None else 0.0,
                            flags))
    if not maps:
        gt = _map(gt, "gt")
        return (torch.zeros((), device=gt.device, dtype=torch.float64 if _fp64 else torch.float32),
                torch.zeros((0, 3), device=gt.device))
    normals = any(M.w_n != 0 for M in maps)
    if normals and target is None:
        target = _target(mono, _map(gt, "gt"), normal_gain, "coarse_loss")
    return loss_terms(maps, gt, valid, maxdisp=maxdisp, target=target if normals else None,
                      gain=gt.shape[-1] / normal_gain, border=side if use_border_mask else "none", lrc_th=lrc_th,
                      _fp64=_fp64)


def coarse_loss(disps, confs, gt, valid, *, maxdisp, side, mono=None, normal_gain=10,
                use_normal_loss_on_coarse=False, use_border_mask=False, lrc_th=1.0):
    """train.py:321-344 (side "left") / 350-377 (side "right") -> the scalar.  ``disps`` / ``confs``: the
    three coarse entries (stereo, mono, scaled mono) of that side, None to skip one.  An entry holding a
    NaN is skipped.  Entry 2 takes its L1 over mask, the others over mask and the side's border mask
    (with ``use_border_mask``) plus 10 times the normals term (with ``use_normal_loss_on_coarse``; the
    reference's stale i_weight is 1); NaN L1 and normals terms are dropped.  The BCE of an entry with a
    confidence is over mask; a NaN one propagates on the left and is dropped on the right."""
    return _coarse(disps, confs, gt, valid, maxdisp=maxdisp, side=side, mono=mono, normal_gain=normal_gain,
                   use_normal_loss_on_coarse=use_normal_loss_on_coarse, use_border_mask=use_border_mask,
                   lrc_th=lrc_th)[0]


def _arg(args, name, default=None):
    if isinstance(args, dict):
        v = args.get(name, default)
    else:
        v = getattr(args, name, default)
    if v is None:
        raise ValueError(f"training_loss: args has no {name}")
    return v


def training_loss(outputs, data, args):
    """train.py:379's total from the six-tuple of ``forward(test_mode=False)`` (pred_disps, pred_confs,
    disps0, disps1, confs0, confs1) and ``data`` (gt, validgt, im2_mono, im3_mono; gt_right and
    validgt_right when the right side has ground truth).  ``args``: a namespace or dict with maxdisp,
    lrc_th, normal_gain, use_normal_loss, use_normal_loss_on_coarse, use_border_mask (the last three
    default to False, normal_gain to 10, lrc_th to 1).  -> (total, terms): terms maps "sequence", "left"
    and "right" to detached [K,3] tensors (L1, normals, BCE per map of that block) and "total"."""
    pred_disps, pred_confs, disps0, disps1, confs0, confs1 = outputs
    maxdisp, lrc_th = _arg(args, "maxdisp"), _arg(args, "lrc_th", 1.0)
    gain = _arg(args, "normal_gain", 10)
    n_seq, n_coarse = bool(_arg(args, "use_normal_loss", False)), bool(_arg(args, "use_normal_loss_on_coarse", False))
    border = bool(_arg(args, "use_border_mask", False))
    if pred_confs is not None and all(c is None for c in pred_confs):
        pred_confs = None
    gt, valid = data["gt"], data["validgt"]
    t_left = _target(data["im2_mono"], _map(gt, "gt"), gain, "training_loss") if (n_seq or n_coarse) else None
    terms = {}
    total, terms["sequence"] = _sequence(pred_disps, gt, valid, maxdisp=maxdisp, normal_gain=gain,
                                         use_normal_loss=n_seq, pred_confs=pred_confs, lrc_th=lrc_th, target=t_left,
                                         _fp64=True)
    t, terms["left"] = _coarse(disps0, confs0, gt, valid, maxdisp=maxdisp, side="left", normal_gain=gain,
                               use_normal_loss_on_coarse=n_coarse, use_border_mask=border, lrc_th=lrc_th,
                               target=t_left, _fp64=True)
    total = total + t
    if "gt_right" in data:
        gtr = data["gt_right"]
        t_right = _target(data["im3_mono"], _map(gtr, "gt_right"), gain, "training_loss") if n_coarse else None
        t, terms["right"] = _coarse(disps1, confs1, gtr, data["validgt_right"], maxdisp=maxdisp, side="right",
                                    normal_gain=gain, use_normal_loss_on_coarse=n_coarse, use_border_mask=border,
                                    lrc_th=lrc_th, target=t_right, _fp64=True)
        total = total + t
    total = total.float()   # the three float64 totals added, rounded once
    terms["total"] = total.detach()
    return total, terms

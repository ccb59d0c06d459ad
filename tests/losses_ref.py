"""A torch restatement of the fused training loss (include/stereoanywhere_hip.h, "The fused training
loss"; train.py:281-379), dtype-generic: in float32 it is the reference formulation, in float64 the
yardstick of tests/test_gpu_losses.py.  Inputs are fp32 numpy arrays or CPU tensors; everything is
cast to ``dtype`` first.  Test infrastructure: it shares no code with stereoanywhere_amd.losses."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

SEL_MASK, SEL_MASK_BORDER = 0, 1


@dataclass
class Map:
    """One map of the fused loss and its constants (the fields of SaLossMap)."""
    map: object
    conf: object = None
    sign: int = 1
    sel: int = SEL_MASK
    w_l1: float = 0.0
    w_n: float = 0.0
    w_bce: float = 0.0
    skip_if_nan_map: bool = False
    drop_nan_l1: bool = False
    drop_nan_bce: bool = False


def _t(a, dtype):
    if a is None:
        return None
    a = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.detach().cpu()
    return a.to(dtype)


# ------------------------------------------------------------------ the reference's three functions
def normalize(x, eps=1e-4):
    """utils.py:56-71 for one tensor: per-sample min / max over the plane, detached."""
    mn = x.amin((2, 3), keepdim=True).detach()
    mx = x.amax((2, 3), keepdim=True).detach()
    return (x - mn) / (mx - mn + eps)


def estimate_normals(depth, normal_gain):
    """utils.py:73-77 with kornia's spatial_gradient(mode='diff', order=1, normalized=False) restated as
    oracle/ops_ref.py spatial_gradient_diff does: replicate pad, right minus left, not halved."""
    p = F.pad(normal_gain * depth, [1, 1, 1, 1], mode="replicate")
    gx = p[:, :, 1:-1, 2:] - p[:, :, 1:-1, :-2]
    gy = p[:, :, 2:, 1:-1] - p[:, :, :-2, 1:-1]
    n = torch.cat([-gx, -gy, torch.ones_like(gx)], 1)
    return n / torch.linalg.norm(n, dim=1, keepdim=True)


def correlation_score(a, b):
    """utils.py:285-293."""
    return torch.sum(a * b, dim=1, keepdim=True)


# ----------------------------------------------------------------------------------- the terms
def selections(gt, valid, maxdisp, border):
    """(mask, mask and border) as train.py:282, 319, 348 build them."""
    mask = (valid > 0) & (gt < maxdisp)
    W = gt.shape[-1]
    col = torch.arange(W, dtype=gt.dtype, device=gt.device).reshape(1, 1, 1, W)
    if border == "left":
        bm = col - gt >= 0
    elif border == "right":
        bm = col + gt < W
    else:
        assert border == "none", border
        bm = torch.ones_like(mask)
    return mask, mask & bm


def _clip01(c):
    """clip(c, 0, 1) with zero slope outside [0, 1] and at 0 and 1."""
    inside = (c > 0) & (c < 1)
    return torch.where(inside, c, c.detach().clamp(0, 1))


def bce_term(m, conf, gt, mask, lrc_th):
    """train.py:338-344 with binary_cross_entropy written out (its logs clamped at -100)."""
    e = (m[mask] - gt[mask]).abs()
    tgt = F.softplus(lrc_th - e).detach() / math.log(1 + math.exp(lrc_th))
    c = conf[mask]
    ok = ~torch.isnan(tgt) & ~torch.isnan(c)
    c, tgt = _clip01(c[ok]), tgt[ok].clamp(0, 1)
    return -(tgt * torch.log(c).clamp(min=-100) + (1 - tgt) * torch.log(1 - c).clamp(min=-100)).mean()


def loss_terms(maps, gt, valid, maxdisp, target=None, gain=1.0, border="none", lrc_th=1.0):
    """total, [(L1_k, N_k, BCE_k)] of torch tensors already in one dtype; a term that is not computed
    (zero weight, skipped map) is None."""
    mask, mask_b = selections(gt, valid, maxdisp, border)
    live, terms = [], []
    for M in maps:
        if M.skip_if_nan_map and torch.isnan(M.map).any():
            terms.append((None, None, None))
            continue
        sel = mask_b if M.sel == SEL_MASK_BORDER else mask
        x = M.sign * M.map
        l1 = n = bce = None
        if M.w_l1 != 0:
            l1 = (x[sel] - gt[sel]).abs().mean()
            if not (M.drop_nan_l1 and torch.isnan(l1)):
                live.append(M.w_l1 * l1)
        if M.w_n != 0:
            n = (1 - correlation_score(estimate_normals(normalize(x), gain), target))[sel].mean()
            if not torch.isnan(n):
                live.append(M.w_n * n)
        if M.w_bce != 0:
            bce = bce_term(M.map, M.conf, gt, mask, lrc_th)
            if not (M.drop_nan_bce and torch.isnan(bce)):
                live.append(M.w_bce * bce)
        terms.append((l1, n, bce))
    total = sum(live) if live else torch.zeros((), dtype=gt.dtype, device=gt.device)
    return total, terms


def loss_and_grads(maps, gt, valid, maxdisp, target=None, gain=1.0, border="none", lrc_th=1.0,
                   dtype=torch.float64, upstream=1.0):
    """The restatement in ``dtype`` from fp32 inputs -> (total, terms [K,3], grad_maps, grad_confs) as
    float64 numpy (terms: 0 where not computed; a confidence-less map's grad_conf is None).  A NaN
    total gives zero gradients."""
    gt, valid, target = _t(gt, dtype), _t(valid, dtype), _t(target, dtype)
    leaves = []
    for M in maps:
        m = _t(M.map, dtype).requires_grad_(True)
        c = None if M.conf is None else _t(M.conf, dtype).requires_grad_(True)
        leaves.append(Map(**{**M.__dict__, "map": m, "conf": c}))
    total, terms = loss_terms(leaves, gt, valid, maxdisp, target, gain, border, lrc_th)
    if total.requires_grad and not torch.isnan(total):
        (total * upstream).backward()
    z = lambda t: None if t is None else (np.zeros(t.shape) if t.grad is None else t.grad.double().numpy())
    vals = np.array([[0.0 if v is None else float(v.detach().double()) for v in row] for row in terms])
    return float(total.detach().double()), vals, [z(M.map) for M in leaves], [z(M.conf) for M in leaves]


# ------------------------------------------------------- train.py's three blocks as lists of maps
def sequence_maps(pred_disps, *, use_normal_loss=False, loss_gamma=0.9, pred_confs=None):
    """train.py:290-316: sign -1, L1 over mask with i_weight, normals with 10 i_weight, and where a
    prediction has a confidence its BCE (309: against the map itself) with i_weight, dropped if NaN."""
    n = len(pred_disps)
    if n < 2:
        raise ValueError("train.py:295 divides by n_predictions - 1")
    out = []
    for i, p in enumerate(pred_disps):
        w = (loss_gamma ** (15 / (n - 1))) ** (n - i - 1)
        conf = None if pred_confs is None else pred_confs[i]
        out.append(Map(p, conf, sign=-1, sel=SEL_MASK, w_l1=w, w_n=10 * w if use_normal_loss else 0.0,
                       w_bce=w if conf is not None else 0.0, drop_nan_bce=True))
    return out


def coarse_maps(disps, confs, *, side, use_normal_loss_on_coarse=False):
    """train.py:321-344 (left) / 350-377 (right)."""
    out = []
    for i, (d, c) in enumerate(zip(disps, confs)):
        if d is None:
            continue
        out.append(Map(d, c, sign=1, sel=SEL_MASK if i == 2 else SEL_MASK_BORDER, w_l1=1.0,
                       w_n=10.0 if (use_normal_loss_on_coarse and i != 2) else 0.0,
                       w_bce=1.0 if c is not None else 0.0, skip_if_nan_map=True, drop_nan_l1=True,
                       drop_nan_bce=(side == "right")))
    return out


def training_calls(outputs, data, args, targets=None):
    """The three loss_terms calls train.py:281-379 amounts to -> [(maps, kwargs)].  args: a dict with
    maxdisp, lrc_th, normal_gain, use_normal_loss, use_normal_loss_on_coarse, use_border_mask.
    targets: (left, right) target normals to use in place of estimate_normals of the mono maps."""
    pred_disps, pred_confs, disps0, disps1, confs0, confs1 = outputs
    W = data["gt"].shape[-1]
    gain = W / args["normal_gain"]
    normals = args["use_normal_loss"] or args["use_normal_loss_on_coarse"]
    border = args["use_border_mask"]

    def tgt(i, key):
        if not normals:
            return None
        return targets[i] if targets is not None else ("mono", key)

    common = dict(maxdisp=args["maxdisp"], gain=gain, lrc_th=args["lrc_th"])
    calls = [(sequence_maps(pred_disps, use_normal_loss=args["use_normal_loss"], pred_confs=pred_confs),
              dict(gt="gt", valid="validgt", target=tgt(0, "im2_mono"), border="none", **common)),
             (coarse_maps(disps0, confs0, side="left", use_normal_loss_on_coarse=args["use_normal_loss_on_coarse"]),
              dict(gt="gt", valid="validgt", target=tgt(0, "im2_mono"), border="left" if border else "none", **common))]
    if "gt_right" in data:
        calls.append((coarse_maps(disps1, confs1, side="right",
                                  use_normal_loss_on_coarse=args["use_normal_loss_on_coarse"]),
                      dict(gt="gt_right", valid="validgt_right", target=tgt(1, "im3_mono"),
                           border="right" if border else "none", **common)))
    return [(m, k) for m, k in calls if m]


def training_loss_and_grads(outputs, data, args, dtype=torch.float64, targets=None):
    """train.py:379's total in ``dtype`` -> (total, [terms per call], grads of every map in the order
    pred_disps, disps0, disps1 (None entries left out), grads of every confidence likewise)."""
    total, terms, gmaps, gconfs = 0.0, [], [], []
    tensors = []
    for maps, kw in training_calls(outputs, data, args, targets):
        gt, valid = _t(data[kw.pop("gt")], dtype), _t(data[kw.pop("valid")], dtype)
        target = kw.pop("target")
        if isinstance(target, tuple):
            target = estimate_normals(_t(data[target[1]], dtype), kw["gain"])
        else:
            target = _t(target, dtype)
        leaves = []
        for M in maps:
            m = _t(M.map, dtype).requires_grad_(True)
            c = None if M.conf is None else _t(M.conf, dtype).requires_grad_(True)
            leaves.append(Map(**{**M.__dict__, "map": m, "conf": c}))
        t, tr = loss_terms(leaves, gt, valid, kw["maxdisp"], target, kw["gain"], kw["border"], kw["lrc_th"])
        total = total + t
        terms.append(np.array([[0.0 if v is None else float(v.detach().double()) for v in row] for row in tr]))
        tensors.append(leaves)
    if not torch.isnan(total):
        total.backward()
    z = lambda t: np.zeros(t.shape) if t.grad is None else t.grad.double().numpy()
    for leaves in tensors:
        gmaps += [z(M.map) for M in leaves]
        gconfs += [z(M.conf) for M in leaves if M.conf is not None]
    return float(total.detach().double()), terms, gmaps, gconfs


# --------------------------------------------------------------------------------- test inputs
def make_case(B, H, W, K, seed, constant_plane=True):
    """Seeded fp32 inputs away from the kinks: |x - gt| >= 0.05, gt at least 0.01 from every integer
    (so from maxdisp, an integer, and from both border conditions), confidences in [0.05, 0.95].
    Sample b's maps are scaled differently (different mn / mx); map 0's last sample is a constant plane
    (mx = mn) unless ``constant_plane`` is off.
    -> dict(gt, valid, maxdisp, mono, maps [K] (the maps themselves: sign * x), confs [K], signs [K])."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    gt = rng.uniform(0.05, max(1.0, 0.6 * W), (B, 1, H, W))
    gt = (np.floor(gt) + np.clip(gt - np.floor(gt), 0.01, 0.99)).astype(f32)
    valid = (rng.uniform(size=gt.shape) < 0.8).astype(f32)
    maxdisp = float(max(1, round(0.45 * W)))
    mono = rng.uniform(0.0, 1.0, gt.shape).astype(f32)
    maps, confs, signs = [], [], []
    for k in range(K):
        sign = -1 if (k % 3 == 0) else 1
        noise = rng.uniform(0.05, 2.0, gt.shape) * rng.choice([-1.0, 1.0], gt.shape)
        noise *= (1.0 + np.arange(B)).reshape(B, 1, 1, 1)
        x = (gt + noise).astype(f32)
        if k == 0 and constant_plane:
            x[B - 1] = -5.0
        maps.append((sign * x).astype(f32))
        confs.append(rng.uniform(0.05, 0.95, gt.shape).astype(f32))
        signs.append(sign)
    return dict(gt=gt, valid=valid, maxdisp=maxdisp, mono=mono, maps=maps, confs=confs, signs=signs)


def check_case(case, border="none"):
    """The preconditions above, for all pixels."""
    gt = case["gt"].astype(np.float64)
    W = gt.shape[-1]
    col = np.arange(W).reshape(1, 1, 1, W)
    assert (np.abs(gt - case["maxdisp"]) >= 1e-3).all()
    assert (np.abs(col - gt) >= 1e-3).all() and (np.abs(col + gt - W) >= 1e-3).all()
    for m, c, s in zip(case["maps"], case["confs"], case["signs"]):
        assert (np.abs(s * m.astype(np.float64) - gt) >= 1e-3).all()
        assert (np.abs(m.astype(np.float64) - gt) >= 1e-3).all()   # the BCE's e is of the map itself
        assert (c >= 0.05).all() and (c <= 0.95).all()

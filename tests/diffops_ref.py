"""Restatements of the five reference formulas the differentiable ops replace (soft-argmin disparity
and entropy confidence, left and right; convex up-sampling), written from the math in
include/stereoanywhere_hip.h:

  * torch, in the dtype of the input (float64: the reference of the GPU tests; float32: the yardstick
    e_ref = max |grad_fp32 - grad_fp64| their tolerance is a multiple of), differentiated by
    torch.autograd;
  * the closed-form gradients in numpy float64, which are what the HIP kernels implement
    (tests/test_diffops_ref_cpu.py holds the two against each other).

Volumes are [B,H,W1,W2] (j over W1, k over W2)."""
import math

import numpy as np
import torch

EPS = 1e-6


# ----------------------------------------------------------------------------------- torch
def left_disparity(vol):
    k = torch.arange(vol.shape[3], dtype=vol.dtype, device=vol.device)
    j = torch.arange(vol.shape[2], dtype=vol.dtype, device=vol.device)
    return j - (torch.softmax(vol, dim=3) * k).sum(3)


def right_disparity(vol):
    k = torch.arange(vol.shape[3], dtype=vol.dtype, device=vol.device)
    j = torch.arange(vol.shape[2], dtype=vol.dtype, device=vol.device)
    return (torch.softmax(vol, dim=2) * j[:, None]).sum(2) - k


def left_confidence(vol):
    p = torch.softmax(vol, dim=3)
    return 1 - (-(p * torch.log2(p + EPS)).sum(3) / math.log2(vol.shape[3]))


def right_confidence(vol):
    q = torch.softmax(vol, dim=2)
    return 1 - (-(q * torch.log2(q + EPS)).sum(2) / math.log2(vol.shape[2]))


def convex_upflow(flow, mask, f, use_scale_factor=True):
    """flow [B,1,H,W], mask [B,9 f f,H,W] -> [B,1,fH,fW]."""
    B, _, H, W = flow.shape
    s = torch.softmax(mask.reshape(B, 9, f, f, H, W), dim=1)
    u = torch.nn.functional.pad(f * flow if use_scale_factor else flow, (1, 1, 1, 1))
    taps = torch.stack([u[:, 0, t // 3:t // 3 + H, t % 3:t % 3 + W] for t in range(9)], dim=1)   # [B,9,H,W]
    up = (s * taps[:, :, None, None]).sum(1)                 # [B,f,f,H,W]
    return up.permute(0, 3, 1, 4, 2).reshape(B, 1, f * H, f * W)


def softargmin_grads(vol_disp, vol_conf, g, dtype):
    """torch.autograd of sum_i <g_i, output_i> in ``dtype``; g = (g_dL, g_dR, g_cL, g_cR), None: that
    output is not used.  -> (grad_vol_disp, grad_vol_conf) as float64 numpy, None without a gradient."""
    out = []
    fns = ((left_disparity, right_disparity), (left_confidence, right_confidence))
    for vol, fn, gs in zip((vol_disp, vol_conf), fns, (g[:2], g[2:])):
        if vol is None or all(x is None for x in gs):
            out.append(None)
            continue
        v = torch.as_tensor(vol).to(dtype).requires_grad_()
        loss = sum((f(v) * torch.as_tensor(x).to(dtype)).sum() for f, x in zip(fn, gs) if x is not None)
        loss.backward()
        out.append(v.grad.double().numpy())
    return tuple(out)


def convex_grads(flow, mask, gout, f, use_scale_factor, dtype):
    """(grad_flow, grad_mask) of <gout, convex_upflow(flow, mask)> in ``dtype``, as float64 numpy."""
    fl = torch.as_tensor(flow).to(dtype).requires_grad_()
    mk = torch.as_tensor(mask).to(dtype).requires_grad_()
    (convex_upflow(fl, mk, f, use_scale_factor) * torch.as_tensor(gout).to(dtype)).sum().backward()
    return fl.grad.double().numpy(), mk.grad.double().numpy()


# ------------------------------------------------------------------- closed forms, numpy float64
def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def _ent_slope(p):
    return np.log2(p + EPS) + p / ((p + EPS) * np.log(2.0))


def closed_softargmin(vol_disp, vol_conf, g):
    """The header's formulas: (grad_vol_disp, grad_vol_conf), None for a volume without a gradient."""
    g_dL, g_dR, g_cL, g_cR = (None if x is None else np.asarray(x, np.float64) for x in g)
    gd = gc = None
    if vol_disp is not None and (g_dL is not None or g_dR is not None):
        v = np.asarray(vol_disp, np.float64)
        W1, W2 = v.shape[2:]
        j, k = np.arange(W1)[:, None], np.arange(W2)[None, :]
        gd = np.zeros_like(v)
        if g_dL is not None:
            p = _softmax(v, 3)
            gd += -g_dL[..., None] * p * (k - (p * k).sum(3, keepdims=True))
        if g_dR is not None:
            q = _softmax(v, 2)
            gd += g_dR[:, :, None, :] * q * (j - (q * j).sum(2, keepdims=True))
    if vol_conf is not None and (g_cL is not None or g_cR is not None):
        v = np.asarray(vol_conf, np.float64)
        W1, W2 = v.shape[2:]
        gc = np.zeros_like(v)
        if g_cL is not None:
            p = _softmax(v, 3)
            a = _ent_slope(p)
            gc += g_cL[..., None] * p * (a - (p * a).sum(3, keepdims=True)) / math.log2(W2)
        if g_cR is not None:
            q = _softmax(v, 2)
            a = _ent_slope(q)
            gc += g_cR[:, :, None, :] * q * (a - (q * a).sum(2, keepdims=True)) / math.log2(W1)
    return gd, gc


def closed_convex(flow, mask, gout, f, scale):
    """(grad_flow [B,1,H,W], grad_mask [B,9 f f,H,W]) by the header's formulas."""
    flow, mask, gout = (np.asarray(a, np.float64) for a in (flow, mask, gout))
    B, _, H, W = flow.shape
    s = _softmax(mask.reshape(B, 9, f, f, H, W), 1)
    g = gout.reshape(B, H, f, W, f).transpose(0, 2, 4, 1, 3)          # [B,a,b,H,W]
    fp = np.pad(flow[:, 0], ((0, 0), (1, 1), (1, 1)))
    u = scale * np.stack([fp[:, t // 3:t // 3 + H, t % 3:t % 3 + W] for t in range(9)], 1)   # [B,9,H,W]
    dot = (s * u[:, :, None, None]).sum(1, keepdims=True)
    g_mask = (s * (u[:, :, None, None] - dot) * g[:, None]).reshape(B, 9 * f * f, H, W)
    c = (s * g[:, None]).sum((2, 3))                                   # [B,9,H,W]: sum over a, b
    g_flow = np.zeros((B, H + 2, W + 2))
    for t in range(9):   # pixel (y', x') sends c_t to (y' + t/3 - 1, x' + t%3 - 1); the border falls off
        g_flow[:, t // 3:t // 3 + H, t % 3:t % 3 + W] += c[:, t]
    return scale * g_flow[:, None, 1:H + 1, 1:W + 1], g_mask

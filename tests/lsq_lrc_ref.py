"""Restatements of the two reference formulas the differentiable softlrc / weighted_lsq replace,
written from the math in include/stereoanywhere_hip.h:

  * torch, in the dtype asked for (float64: the reference of the GPU tests; float32: the yardstick
    e_ref = max |grad_fp32 - grad_fp64| their tolerance is a multiple of), differentiated by
    torch.autograd (the warp through torch's grid_sample, the solve through torch.linalg.lstsq);
  * the closed-form gradients in numpy float64, which are what the HIP kernels implement
    (tests/test_lsq_lrc_ref_cpu.py holds the two against each other).

Disparity / confidence maps are [B,1,H,W]; weighted_lsq maps [B, n]."""
import math

import numpy as np
import torch
import torch.nn.functional as F


# ----------------------------------------------------------------------------------- torch
def warp(src_disp, img, right):
    """img sampled at x + src_disp (right) or x - src_disp: the grid is normalised by W and H and
    sampled with align_corners=True, bilinear, zero padding."""
    B, _, H, W = img.shape
    xs = torch.arange(W, dtype=img.dtype, device=img.device).view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H, dtype=img.dtype, device=img.device).view(1, H, 1).expand(B, H, W)
    xn = xs + src_disp[:, 0] if right else xs - src_disp[:, 0]
    grid = torch.stack([2 * (xn / W) - 1, 2 * (ys / H) - 1], dim=3)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def softlrc(d2, d3, c2=None, c3=None, th=1.0):
    """(s2, s3): softplus(th - |d - warped other|) / log(1 + e^th), times the confidence if given."""
    div = math.log(1 + math.exp(th))
    s2 = F.softplus(th - (d2 - warp(torch.relu(d2), d3, False)).abs()) / div
    s3 = F.softplus(th - (d3 - warp(torch.relu(d3), d2, True)).abs()) / div
    return (s2 if c2 is None else c2 * s2), (s3 if c3 is None else c3 * s3)


def softlrc_grads(d2, d3, c2, c3, th, g2, g3, dtype):
    """torch.autograd of <g2, s2> + <g3, s3> in ``dtype`` (a None g: that output is not used)
    -> (grad_d2, grad_d3, grad_c2, grad_c3) as float64 numpy, None for an absent confidence."""
    t = [None if a is None else torch.as_tensor(a).to(dtype).requires_grad_() for a in (d2, d3, c2, c3)]
    s2, s3 = softlrc(*t, th=th)
    loss = sum((s * torch.as_tensor(g).to(dtype)).sum() for s, g in ((s2, g2), (s3, g3)) if g is not None)
    loss.backward()
    return tuple(None if a is None else (torch.zeros_like(a) if a.grad is None else a.grad).double().numpy()
                 for a in t)


def band(disp32, q_lo=0.2, q_hi=0.9):
    """The reference's band of one sample: torch.quantile of the fp32 relu'd values, and the inclusive
    membership mask (compared in fp32).  disp32: a float32 tensor [n]."""
    y = torch.relu(disp32.float())
    lo, hi = torch.quantile(y, q_lo), torch.quantile(y, q_hi)
    return lo, hi, (lo <= y) & (y <= hi)


def weighted_lsq(mde, disp, conf, dtype, q_lo=0.2, q_hi=0.9):
    """The reference's formulation per sample: the band from the fp32 values (constants), then
    lstsq([|m| w, w], relu(d) w) with w = sqrt(0.9 |c| + 0.1) in ``dtype``.  mde, disp, conf: float32
    tensors [B, n] or their ``dtype`` copies that carry the graph (exact, so .float() gives the fp32
    values back) -> (scale [B], shift [B])."""
    out = []
    for b in range(mde.shape[0]):
        _, _, keep = band(disp[b].detach())
        m, y, c = mde[b].to(dtype)[keep].abs(), torch.relu(disp[b].to(dtype))[keep].abs(), conf[b].to(dtype)[keep].abs()
        w = torch.sqrt(c * (1 - 0.1) + 0.1)
        A = torch.stack([m * w, w], dim=1)
        out.append(torch.linalg.lstsq(A, (y * w)[:, None]).solution[:, 0])
    sol = torch.stack(out)
    return sol[:, 0], sol[:, 1]


def weighted_lsq_grads(mde, disp, conf, g_scale, g_shift, dtype):
    """torch.autograd of <g_scale, scale> + <g_shift, shift> in ``dtype`` from float32 numpy inputs
    -> (grad_mde, grad_disp, grad_conf) as float64 numpy."""
    m, d, c = (torch.as_tensor(np.asarray(a, np.float32)).to(dtype).requires_grad_() for a in (mde, disp, conf))
    sol = torch.stack(weighted_lsq(m, d, c, dtype), dim=1)
    loss = 0
    if g_scale is not None:
        loss = loss + (sol[:, 0] * torch.as_tensor(g_scale).to(dtype)).sum()
    if g_shift is not None:
        loss = loss + (sol[:, 1] * torch.as_tensor(g_shift).to(dtype)).sum()
    loss.backward()
    return tuple(t.grad.double().numpy() for t in (m, d, c))


# ------------------------------------------------------------------- closed forms, numpy float64
def lrc_coords(d, right):
    """(ix, iy) [B,H,W] float64: the source coordinates pixel (y, x) of a [B,1,H,W] map samples at."""
    d = np.asarray(d, np.float64)[:, 0]
    B, H, W = d.shape
    x = np.arange(W)[None, None, :]
    r = np.maximum(d, 0)
    ix = ((x + r if right else x - r) / W) * (W - 1)
    iy = np.broadcast_to((np.arange(H)[None, :, None] / H) * (H - 1), d.shape)
    return ix, iy


def _side(dself, dother, conf, g, th, right):
    """One map's side: (s, own gradient of dself, tap gradient of dother, gradient of conf, u)."""
    dself, dother = np.asarray(dself, np.float64)[:, 0], np.asarray(dother, np.float64)[:, 0]
    B, H, W = dself.shape
    ix, iy = lrc_coords(dself[:, None], right)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    w, n = ix - x0, iy - y0
    e, s = 1 - w, 1 - n
    bi = np.broadcast_to(np.arange(B)[:, None, None], dself.shape)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
        return np.where(ok, dother[bi, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0.0), ok

    (v00, k00), (v01, k01), (v10, k10), (v11, k11) = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    u = dself - (v00 * s * e + v01 * s * w + v10 * n * e + v11 * n * w)
    z = th - np.abs(u)
    div = math.log(1 + math.exp(th))
    v = np.where(z > 20, z, np.log1p(np.exp(np.minimum(z, 20)))) / div
    cf = 1.0 if conf is None else np.asarray(conf, np.float64)[:, 0]
    out = v * cf
    if g is None:
        return out, np.zeros_like(dself), np.zeros_like(dself), np.zeros_like(dself), u
    g = np.asarray(g, np.float64)[:, 0]
    slope = np.where(z > 20, 1.0, 1 / (1 + np.exp(-z)))
    t = g * cf * (-slope * np.sign(u) / div)
    dS = (v01 - v00) * s + (v11 - v10) * n
    dix = np.where(dself > 0, (1.0 if right else -1.0) * (W - 1) / W, 0.0)
    own = t * (1 - dS * dix)
    taps = np.zeros_like(dother)
    for (yy, xx, wt, ok) in ((y0, x0, s * e, k00), (y0, x0 + 1, s * w, k01), (y0 + 1, x0, n * e, k10),
                             (y0 + 1, x0 + 1, n * w, k11)):
        np.add.at(taps, (bi[ok], yy[ok], xx[ok]), (-t * wt)[ok])
    return out, own, taps, g * v, u


def closed_softlrc(d2, d3, c2, c3, th, g2, g3):
    """The header's formulas -> (s2, s3), (grad_d2, grad_d3, grad_c2, grad_c3) [B,1,H,W] float64 (a
    confidence gradient is None without that confidence)."""
    s2, own2, tap3, gc2, _ = _side(d2, d3, c2, g2, th, False)
    s3, own3, tap2, gc3, _ = _side(d3, d2, c3, g3, th, True)
    grads = (own2 + tap2, own3 + tap3, None if c2 is None else gc2, None if c3 is None else gc3)
    return (s2[:, None], s3[:, None]), tuple(None if a is None else a[:, None] for a in grads)


def closed_weighted_lsq(mde, disp, conf, g_scale, g_shift, q_lo=0.2, q_hi=0.9):
    """The header's formulas from float32 inputs [B, n] -> (scale, shift) [B] and (grad_mde, grad_disp,
    grad_conf) [B, n], float64; the band as the reference takes it (fp32 quantiles, fp32 compares)."""
    m32, d32, c32 = (np.asarray(a, np.float32) for a in (mde, disp, conf))
    B, n = m32.shape
    scale, shift = np.zeros(B), np.zeros(B)
    grads = [np.zeros((B, n)) for _ in range(3)]
    for b in range(B):
        _, _, keep = band(torch.from_numpy(d32[b]), q_lo, q_hi)
        k = keep.numpy().astype(np.float64)
        m, d, c = (a[b].astype(np.float64) for a in (m32, d32, c32))
        a, y, wt = np.abs(m), np.maximum(d, 0), 0.9 * np.abs(c) + 0.1
        N = np.array([[(k * wt * a * a).sum(), (k * wt * a).sum()], [(k * wt * a).sum(), (k * wt).sum()]])
        x = np.linalg.solve(N, np.array([(k * wt * a * y).sum(), (k * wt * y).sum()]))
        g = np.array([0.0 if g_scale is None else float(g_scale[b]), 0.0 if g_shift is None else float(g_shift[b])])
        v = np.linalg.solve(N, g)
        u, r = a * v[0] + v[1], y - (a * x[0] + x[1])
        scale[b], shift[b] = x
        grads[0][b] = np.sign(m) * k * wt * (v[0] * r - u * x[0])
        grads[1][b] = k * wt * u * (d > 0)
        grads[2][b] = 0.9 * np.sign(c) * k * u * r
    return (scale, shift), tuple(grads)


# ------------------------------------------------------------------------- test inputs, softlrc
FRAC_LO, FRAC_HI, MIN_ABS = 0.05, 0.95, 1e-3


def _frac_ok(d, right):
    ix, _ = lrc_coords(d, right)
    fr = ix - np.floor(ix)
    return ((fr >= FRAC_LO) & (fr <= FRAC_HI) & (np.abs(np.asarray(d, np.float64)[:, 0]) >= MIN_ABS))[:, None]


def lrc_precondition(d2, d3):
    """Every sample point's fractional ix in [0.05, 0.95], |u| >= 1e-3 and |d| >= 1e-3 on both maps: away
    from the kinks of bilinear sampling, |u| and relu, where fp32 and fp64 may pick different branches."""
    u2, u3 = _side(d2, d3, None, None, 1.0, False)[4], _side(d3, d2, None, None, 1.0, True)[4]
    return _frac_ok(d2, False) & (np.abs(u2) >= MIN_ABS)[:, None], _frac_ok(d3, True) & (np.abs(u3) >= MIN_ABS)[:, None]


def lrc_inputs(B, H, W, amp, seed):
    """Two float32 disparity maps [B,1,H,W], uniform in [-amp, amp], built with a fixed seed and
    offending pixels redrawn until lrc_precondition holds everywhere.  With amp >= W one pixel of each
    map is planted to sample the half-in border cell past its edge of the plane (ix = -0.5 for the
    left map, W - 0.5 for the right one)."""
    rng = np.random.default_rng(seed)
    d2, d3 = (rng.uniform(-amp, amp, (B, 1, H, W)).astype(np.float32) for _ in range(2))
    fixed2, fixed3 = np.zeros(d2.shape, bool), np.zeros(d3.shape, bool)
    if amp >= W:
        d2[0, 0, 0, 0] = 0.5 * W / (W - 1)              # x = 0:     ix = -0.5 (W - 1) / W (W / (W - 1)) = -0.5
        d3[0, 0, 0, W - 1] = (W - 0.5) * W / (W - 1) - (W - 1)   # x = W - 1: ix = W - 1 + 0.5
        fixed2[0, 0, 0, 0] = fixed3[0, 0, 0, W - 1] = True
    for _ in range(200):
        ok2, ok3 = lrc_precondition(d2, d3)
        bad2, bad3 = ~ok2 & ~fixed2, ~ok3 & ~fixed3
        if not (bad2.any() or bad3.any()):
            break
        d2[bad2] = rng.uniform(-amp, amp, int(bad2.sum())).astype(np.float32)
        d3[bad3] = rng.uniform(-amp, amp, int(bad3.sum())).astype(np.float32)
    return d2, d3


# -------------------------------------------------------------------- test inputs, weighted_lsq
def lsq_inputs(n, kind, seed=0):
    """float32 (mde, disp, conf) [2, n] with negative mde / conf entries, the two samples different.
    kind "random": disp ~ N(3, 4); "zeros": 60 % of disp <= 0 (the lower threshold is 0 and the zero
    keys are inside the band); "ties": disp in steps of 0.25 (many elements equal the band's order
    statistics); "rank": sample 0 with all |mde| equal (the rank-deficient branch)."""
    rng = np.random.default_rng(1000 * n + seed)
    m = (3.0 * rng.standard_normal((2, n))).astype(np.float32)
    d = (4.0 * rng.standard_normal((2, n)) + 3.0).astype(np.float32)
    c = rng.uniform(-1, 1, (2, n)).astype(np.float32)
    if kind == "zeros":
        d = np.where(rng.uniform(size=d.shape) < 0.6, -np.abs(d) * (rng.uniform(size=d.shape) < 0.8),
                     np.abs(d) + 0.5).astype(np.float32)
    elif kind == "ties":
        d = (np.round(d * 4) / 4).astype(np.float32)
    elif kind == "rank":
        m[0] = np.where(m[0] < 0, -1.5, 1.5).astype(np.float32)
    else:
        assert kind == "random", kind
    return m, d, c

"""tests/corr_autograd_ref.py (the float64 restatement of the plug-in's adjoints, in its
float64-coefficient mode) against torch.autograd of the reference formulation in float64 on the
CPU: einsum / sqrt(C), a multiply by a volume T, avg_pool2d([1, 2]) and grid_sample(align_corners=
True) at 2 x / (W_l - 1) - 1 (corr.py:76-132, utils.py:19-35 of the reference)."""
import numpy as np
import torch
import torch.nn.functional as F

import corr_autograd_ref as ref


def _coords(rng, B, H, W, W2, R):
    """[B,1,H,W] covering [-R-3, W2+R+3]: every integer and every .5 of the range among them."""
    lo, hi = -R - 3, W2 + R + 3
    n = B * H * W
    exact = np.arange(lo, hi + 0.25, 0.5)
    assert exact.size < n
    cx = np.concatenate([exact, rng.random(n - exact.size) * (hi - lo) + lo])
    rng.shuffle(cx)
    return cx.reshape(B, 1, H, W)


def _torch_formulation(f2, f3, T, cx, L, R):
    """The taps [B, L (2R+1), H, W1] as the reference model computes them."""
    B, C, H, W1 = f2.shape
    W2 = f3.shape[3]
    vol = torch.einsum("aijk,aijh->ajkh", f2, f3) / torch.sqrt(torch.tensor(float(C), dtype=torch.float64))
    level = (T * vol).reshape(B * H * W1, 1, 1, W2)
    x = cx.permute(0, 2, 3, 1).reshape(B * H * W1, 1, 1, 1)
    dx = torch.linspace(-R, R, 2 * R + 1, dtype=torch.float64).view(1, 1, 2 * R + 1, 1)
    out = []
    for l in range(L):
        Wl = level.shape[-1]
        xg = 2 * (dx + x / 2 ** l) / (Wl - 1) - 1
        grid = torch.cat([xg, torch.zeros_like(xg)], dim=-1)
        out.append(F.grid_sample(level, grid, align_corners=True).view(B, H, W1, -1))
        level = F.avg_pool2d(level, [1, 2], stride=[1, 2])
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2)


def test_helper_matches_torch_autograd():
    """Relative difference (max |a - b| / max |b|) <= 1e-12 for the loss and the three gradients:
    both sides are float64 sums of a few hundred terms (3e-16 measured at this shape); the
    coordinates' grid round trip moves a coefficient by ~1e-16 of a cell, continuously."""
    B, C, H, W1, W2, L, R = 2, 5, 3, 13, 21, 3, 2
    rng = np.random.default_rng(11)
    f2 = rng.standard_normal((B, C, H, W1))
    f3 = rng.standard_normal((B, C, H, W2))
    T = rng.standard_normal((B, H, W1, W2))
    Rw = rng.standard_normal((B, L * (2 * R + 1), H, W1))
    cx = _coords(rng, B, H, W1, W2, R)

    tf2, tf3, tT = (torch.from_numpy(a).requires_grad_() for a in (f2, f3, T))
    taps = _torch_formulation(tf2, tf3, tT, torch.from_numpy(cx), L, R)
    loss = (taps * torch.from_numpy(Rw)).sum()
    loss.backward()

    A = ref.lookup_matrix(cx, W2, L, R)
    sqrt_c = float(np.sqrt(np.float64(C)))
    got_loss, g2, g3, gT = ref.chain(f2, f3, T, A, Rw, L, sqrt_c)

    # the forward pieces too: taps of the helper against the formulation's
    pyr = ref.pyramid_forward((T * ref.volume_forward(f2, f3, sqrt_c)).reshape(-1, W2), L)
    my_taps = ref.lookup_forward(A, pyr).reshape(B, H, W1, -1).transpose(0, 3, 1, 2)
    pairs = [("taps", my_taps, taps.detach().numpy()), ("loss", np.array(got_loss), loss.detach().numpy()),
             ("f2.grad", g2, tf2.grad.numpy()), ("f3.grad", g3, tf3.grad.numpy()), ("T.grad", gT, tT.grad.numpy())]
    for name, a, b in pairs:
        rel = np.abs(a - b).max() / np.abs(b).max()
        print(f"{name}: relative difference {rel:.3g}")
        assert rel <= 1e-12, name
    assert np.abs(tT.grad.numpy()).max() > 0


def test_adjoints_are_transposes():
    """<A p, g> == <p, A^T g> for the scatter and the fold, in float64 (1e-12 relative)."""
    rng = np.random.default_rng(3)
    W2, L, R = 21, 3, 2
    _, _, total = ref.level_geometry(W2, L)
    cx = _coords(rng, 2, 3, 13, W2, R)
    A = ref.lookup_matrix(cx, W2, L, R)
    p = rng.standard_normal((cx.size, total))
    g = rng.standard_normal((2, L * (2 * R + 1), 3, 13))
    lhs = (ref.lookup_forward(A, p) * g.transpose(0, 2, 3, 1).reshape(cx.size, -1)).sum()
    rhs = (p * ref.lookup_backward(A, g)).sum()
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    v = rng.standard_normal((7, W2))
    gp = rng.standard_normal((7, total))
    lhs = (ref.pyramid_forward(v, L) * gp).sum()
    rhs = (v * ref.pyramid_backward(gp, W2, L)).sum()
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)

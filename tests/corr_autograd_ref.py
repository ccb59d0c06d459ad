"""Float64 numpy restatements of the three adjoints of the correlation plug-in and of their chain
(no torch, no GPU): the reference that tests/test_gpu_corr_backward.py compares the HIP backward
kernels against, itself checked against torch.autograd in tests/test_corr_autograd_ref_cpu.py.

Layouts are the library's: a pyramid row holds the levels of one pixel back to back, level l of
width W2 >> l (floored at every halving) at offset sum of the widths before it.

The lookup is linear in the pyramid: tap (l, t) of pixel p is sum_m A[p, l (2r+1) + t + r, m] row_p[m].
``A`` comes either from float64 coordinates (``lookup_matrix``) or is given (the GPU tests extract
the forward kernel's own fp32 coefficients, so that only the backward's rounding is measured)."""
import numpy as np


def level_geometry(W2, L):
    """(offsets, widths, total) of an L-level pyramid row."""
    wids = [W2]
    for _ in range(1, L):
        wids.append(wids[-1] // 2)
    offs = [int(sum(wids[:i])) for i in range(L)]
    return offs, wids, int(sum(wids))


def lookup_matrix(coords_x, W2, L, R):
    """A [npix, L (2R+1), total] from float64 ix = x / 2^l + t: weight 1 - w on cell floor(ix), w on
    the next, a cell outside [0, W_l - 1] dropped.  coords_x: [B,1,H,W1] (pixels in b, h, j order)."""
    x = np.asarray(coords_x, dtype=np.float64).reshape(-1)
    offs, wids, total = level_geometry(W2, L)
    K = 2 * R + 1
    A = np.zeros((x.size, L * K, total))
    p = np.arange(x.size)
    for l in range(L):
        for t in range(-R, R + 1):
            ix = x / 2.0 ** l + t
            xi = np.floor(ix)
            w = ix - xi
            xi = xi.astype(np.int64)
            for cell, coef in ((xi, 1.0 - w), (xi + 1, w)):
                ok = (cell >= 0) & (cell <= wids[l] - 1)
                np.add.at(A, (p[ok], l * K + t + R, offs[l] + cell[ok]), coef[ok])
    return A


def _pixels(g):
    """[B, Q, H, W1] -> [B H W1, Q] float64."""
    g = np.asarray(g, dtype=np.float64)
    return g.transpose(0, 2, 3, 1).reshape(-1, g.shape[1])


def lookup_forward(A, pyramid):
    """taps [npix, L (2R+1)] of pyramid rows [npix, >= total]."""
    return np.einsum("pqm,pm->pq", A, np.asarray(pyramid, dtype=np.float64)[:, :A.shape[2]])


def lookup_backward(A, grad_out):
    """The scatter: grad_pyramid [npix, total] = A^T grad_out, grad_out [B, L (2R+1), H, W1]."""
    return np.einsum("pqm,pq->pm", A, _pixels(grad_out))


def pyramid_forward(volume, L):
    """[rows, W2] -> pyramid rows [rows, total]: each level the mean of the pairs of the one before."""
    v = np.asarray(volume, dtype=np.float64)
    levels = [v]
    for _ in range(1, L):
        w = levels[-1].shape[1] // 2
        levels.append(0.5 * (levels[-1][:, 0:2 * w:2] + levels[-1][:, 1:2 * w:2]))
    return np.concatenate(levels, axis=1)


def pyramid_backward(grad_pyramid, W2, L):
    """The fold: grad_volume[k] = sum_l 2^-l grad_level_l[k >> l] over the levels with (k >> l) < W_l."""
    gp = np.asarray(grad_pyramid, dtype=np.float64)
    offs, wids, _ = level_geometry(W2, L)
    k = np.arange(W2)
    gv = np.zeros((gp.shape[0], W2))
    for l in range(L):
        kl = k >> l
        ok = kl < wids[l]
        gv[:, ok] += 0.5 ** l * gp[:, offs[l] + kl[ok]]
    return gv


def volume_forward(f2, f3, sqrt_c):
    """[B,C,H,W1] x [B,C,H,W2] -> [B,H,W1,W2] / sqrt_c."""
    return np.einsum("bchj,bchk->bhjk", np.asarray(f2, np.float64), np.asarray(f3, np.float64)) / float(sqrt_c)


def volume_backward(grad_volume, f2, f3, sqrt_c):
    """The two GEMMs: (grad_fmap2 [B,C,H,W1], grad_fmap3 [B,C,H,W2])."""
    G = np.asarray(grad_volume, dtype=np.float64)
    g2 = np.einsum("bhjk,bchk->bchj", G, np.asarray(f3, np.float64)) / float(sqrt_c)
    g3 = np.einsum("bhjk,bchj->bchk", G, np.asarray(f2, np.float64)) / float(sqrt_c)
    return g2, g3


def chain(f2, f3, T, A, grad_out, L, sqrt_c):
    """loss = sum(grad_out * lookup(pyramid(T * corr(f2, f3)))) -> (loss, f2.grad, f3.grad, T.grad).
    T: [B,H,W1,W2]; grad_out: [B, L (2R+1), H, W1] (the weights of the sum; zero where the block's
    pad crops the output).  Called on absolute values (every coefficient is non-negative) it
    returns the sums of the absolute terms."""
    f2, f3, T = (np.asarray(a, dtype=np.float64) for a in (f2, f3, T))
    B, _, H, W1 = f2.shape
    W2 = f3.shape[3]
    vol = volume_forward(f2, f3, sqrt_c)
    pyr = pyramid_forward((T * vol).reshape(-1, W2), L)
    loss = float((lookup_forward(A, pyr) * _pixels(grad_out)).sum())
    gv = pyramid_backward(lookup_backward(A, grad_out), W2, L).reshape(B, H, W1, W2)
    g2, g3 = volume_backward(gv * T, f2, f3, sqrt_c)
    return loss, g2, g3, gv * vol

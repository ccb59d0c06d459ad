"""The split F(4x4,3x3) kernel's filter image (sa_conv2d_wino4_weights_split), rebuilt in numpy from
its documented order (include/stereoanywhere_hip.h):

    f16 [Cout/32][Cin/8][36 points][4 k][16 n][2 groups][hi | lo][2 jobs]

for input channel 8 chunk + 4 job + k and output channel 32 block + 16 group + n: one dword holds
the two jobs' hi halves (job 0 in the low half), the next their lo halves, with U = G g G^T in
float64 times 2^12, hi = f16(U), lo = f16(U - hi).  The image is written by a GPU kernel only, so the
test reads it back (gpu-marked despite the file's name, which is the one the change was specified
with)."""
import numpy as np
import pytest
import torch

from stereoanywhere_amd import ops

pytestmark = pytest.mark.gpu

G = np.array([[0.25, 0.0, 0.0], [-1.0 / 6, -1.0 / 6, -1.0 / 6], [-1.0 / 6, 1.0 / 6, -1.0 / 6],
              [1.0 / 24, 1.0 / 12, 1.0 / 6], [1.0 / 24, -1.0 / 12, 1.0 / 6], [0.0, 0.0, 1.0]], dtype=np.float64)


def _expected(w):
    """(image as uint16 [.., hi | lo, job], U * 2^12 in float64 [6, 6, Cout, Cin]): the kernel's
    arithmetic, sums left to right."""
    Cout, Cin = w.shape[:2]
    g = w.astype(np.float64)
    u = np.empty((6, 6, Cout, Cin))
    for a in range(6):
        t = [G[a, 0] * g[:, :, 0, c] + G[a, 1] * g[:, :, 1, c] + G[a, 2] * g[:, :, 2, c] for c in range(3)]
        for b in range(6):
            u[a, b] = (t[0] * G[b, 0] + t[1] * G[b, 1] + t[2] * G[b, 2]) * 4096.0
    hi = u.astype(np.float32).astype(np.float16)
    lo = (u - hi.astype(np.float64)).astype(np.float32).astype(np.float16)
    img = np.empty((Cout // 32, Cin // 8, 36, 4, 16, 2, 2, 2), np.uint16)
    # [a, b, co, ci] -> [cb, gg, n | chunk, s, k] -> [cb, chunk, pt, k, n, gg, (hi | lo), s]
    for half, v in enumerate((hi, lo)):
        r = v.view(np.uint16).reshape(36, Cout // 32, 2, 16, Cin // 8, 2, 4)   # pt, cb, gg, n, chunk, s, k
        img[..., half, :] = r.transpose(1, 4, 0, 6, 3, 2, 5)
    return img, u


@pytest.mark.parametrize("Cin", [8, 16])
@pytest.mark.parametrize("Cout", [32, 64])
def test_split_image_order_and_pairs(monkeypatch, Cin, Cout):
    monkeypatch.setattr(ops, "W4_SPLIT", True)
    w = (np.random.default_rng(Cin + Cout).standard_normal((Cout, Cin, 3, 3)) * 0.2).astype(np.float32)
    U = ops.wino_weights(torch.from_numpy(w).cuda())
    assert U.u4s is not None and U.u4s.numel() == 36 * Cin * Cout
    got = U.u4s.cpu().numpy().view(np.uint32)
    img, u = _expected(w)
    exp = img.reshape(-1).view(np.uint32)   # (little-endian: the first f16 of a pair is the dword's low half)
    bad = np.flatnonzero(got != exp)
    # Dword for dword, with one freedom.  U = (sum of filter taps) * 2^12 / 3, / 9, ... is often a short
    # binary fraction, so a residual U - hi lies EXACTLY on an f16 rounding tie in about 1 % of the
    # values (and U itself in about 1 of 10^4); which neighbour the half then takes is decided by the
    # last bit of the fp64 sums (whether the compiler fused their multiply-adds).  Such a half may be
    # the other neighbour: a hi half as near to U as numpy's, to 2^-30 of U, and a lo half as near to
    # the float64 residual of ITS hi half as that residual's own rounding, to 2^-30 of it.  Every
    # other half matches bit for bit (the nearest f16 is unique), and no more than 3 % of the dwords
    # may use the freedom.
    assert bad.size <= 0.03 * got.size, bad.size

    def image_order(v):   # [6, 6, Cout, Cin] -> [cb, chunk, pt, k, n, gg, s]
        return v.reshape(36, Cout // 32, 2, 16, Cin // 8, 2, 4).transpose(1, 4, 0, 6, 3, 2, 5)
    g16 = got.view(np.uint16).reshape(img.shape).view(np.float16).astype(np.float64)
    e16 = img.view(np.float16).astype(np.float64)
    ui = image_order(u)
    assert (np.abs(g16[..., 0, :] - ui) <= np.abs(e16[..., 0, :] - ui) + 2.0 ** -30 * np.abs(ui)).all()
    resid = ui - g16[..., 0, :]
    near = resid.astype(np.float32).astype(np.float16).astype(np.float64)
    d_got, d_near = np.abs(g16[..., 1, :] - resid), np.abs(near - resid)
    assert (d_got <= d_near + 2.0 ** -30 * np.abs(resid)).all(), float((d_got - d_near).max())
    # every (hi, lo) pair of the image stands for its U * 2^12: to 2^-22 relative in the f16 normal
    # range of lo (|U 2^12| >= 2^-3), to an absolute 2^-25 below (test_split_numerics_cpu.py)
    pairs = got.view(np.uint16).reshape(Cout // 32, Cin // 8, 36, 4, 16, 2, 2, 2).view(np.float16).astype(np.float64)
    s = (pairs[..., 0, :] + pairs[..., 1, :]).transpose(2, 0, 5, 4, 1, 6, 3).reshape(6, 6, Cout, Cin)
    # (the residual U - hi goes through fp32 on its way to f16: 2^-24 of a value below 2^-3 * 2^-11 on
    # top of the half spacing 2^-25 of a subnormal lo)
    big = np.abs(u) >= 2.0 ** -3
    assert big.any()
    assert (np.abs(s - u)[big] / np.abs(u[big])).max() <= 2.0 ** -22
    if (~big).any():
        assert np.abs(s - u)[~big].max() <= 2.0 ** -25 + 2.0 ** -38

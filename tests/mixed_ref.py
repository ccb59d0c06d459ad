"""The mixed-precision F(4x4,3x3) conv (conv2d_wino4.hip W4Half, block_shape 7) restated in numpy,
beside test_split_numerics_cpu.py's ``wino4``: the fp32 transformed input rounded ONCE to f16,
hi = f16(V); the filters the exact f16 pairs split16(U * 4096), both halves used; products exact,
sums fp32; / 4096; fp32 output transform.  Shared by test_mixed_numerics_cpu.py and
test_gpu_wino_mixed.py (the kernel's reference value)."""
import numpy as np

from test_split_numerics_cpu import AT, BT, G, direct, split16


def wino4_mixed(x, w):
    """3x3 / pad 1 conv of x [Cin, H, W] (W % 4 == 0; H zero-padded to a multiple of 4, as the
    kernel's tiles do) by w [Cout, Cin, 3, 3] -> [Cout, H, W] fp32."""
    cin, H, W = x.shape
    Hp = (H + 3) // 4 * 4
    assert W % 4 == 0
    xp = np.pad(x, ((0, 0), (1, 1 + Hp - H), (1, 1)))
    U = np.einsum("ak,oikl,bl->abio", G, w.astype(np.float64), G).astype(np.float32)
    th, tw = Hp // 4, W // 4
    d = np.stack([np.stack([xp[:, 4 * i:4 * i + 6, 4 * j:4 * j + 6] for j in range(tw)], 1) for i in range(th)], 1)
    V = np.einsum("ak,ctskl,bl->abcts", BT.astype(np.float32), d, BT.astype(np.float32)).astype(np.float32)
    vh = V.astype(np.float16).astype(np.float32)
    uh, ul = split16(U * np.float32(4096))
    M = np.einsum("abcts,abco->abots", vh, uh, dtype=np.float32)
    M += np.einsum("abcts,abco->abots", vh, ul, dtype=np.float32)
    M /= np.float32(4096)
    Y = np.einsum("ia,abots,jb->otisj", AT.astype(np.float32), M, AT.astype(np.float32))
    return Y.reshape(w.shape[0], Hp, W)[:, :H]


def direct_f16_operands(x, w):
    """Direct conv with x and w each rounded to f16 (what autocast's f16 conv is given), summed in fp64."""
    return direct(x.astype(np.float16).astype(np.float32), w.astype(np.float16).astype(np.float32))


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))

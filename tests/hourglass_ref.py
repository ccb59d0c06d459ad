"""Float64 CPU reference of the fused hourglass's stages (csrc/conv3d_fused.hip, conv3d_mfma.hip,
conv3d_s2mf.hip), one plain torch function per stage, on the [B, C, D = W2, H, W = W1] layout.
Every result comes with its magnitude ``mag``: the same computation on absolute values, the scale
of a rounding-error bound.  Independent of the HIP kernels and of their Python wrappers;
tests/test_hourglass_ref_cpu.py pins it to the torch Hourglass module.
Reference: hourglass.py:13-91, submodule.py:25-53 (BasicConv3d), :113-140 (DoubleFeatureAtt)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ops_ref as R

U = 2.0 ** -24   # unit roundoff of float32


def T(x, norm=None, act=False, gate=None, slope=0.01):
    """The transform a consumer applies on load: (x - mean) * rstd, LeakyReLU, then the gate
    gl[b,c,h,w] * gr[b,c,h,d] (blocks.DoubleFeatureAtt.forward)."""
    x = x.double()
    B, C, D, H, W = x.shape
    if norm is not None:
        mean, rstd = (t.double().reshape(B, C, 1, 1, 1) for t in norm)
        x = (x - mean) * rstd
    if act:
        x = F.leaky_relu(x, slope)
    if gate is not None:
        gl, gr = gate[0].double().reshape(B, C, H, W), gate[1].double().reshape(B, C, H, D)
        x = x * gl[:, :, None] * gr.permute(0, 1, 3, 2)[..., None]
    return x


def _k3(w_t):
    cin, _, cout = w_t.shape
    return w_t.double().reshape(cin, 3, 3, 3, cout).permute(4, 0, 1, 2, 3)


def conv3(tx, w_t, stride=1):
    """3x3x3 conv, zero padding 1 of the transformed input, weights [Cin][27][Cout] -> (out, mag)."""
    w = _k3(w_t)
    return F.conv3d(tx, w, stride=stride, padding=1), F.conv3d(tx.abs(), w.abs(), stride=stride, padding=1)


def pointwise(tx, w):
    """1x1x1 conv, weights [Cin][Cout] -> (out, mag)."""
    w = w.double()
    return torch.einsum("bcdhw,co->bodhw", tx, w), torch.einsum("bcdhw,co->bodhw", tx.abs(), w.abs())


def stats(y, eps=1e-5):
    """InstanceNorm3d statistics per (b, c), flattened: mean and rstd of the biased variance."""
    y = y.double()
    mean = y.mean(dim=(2, 3, 4))
    var = ((y - mean[:, :, None, None, None]) ** 2).mean(dim=(2, 3, 4))
    return mean.reshape(-1), (1.0 / torch.sqrt(var + eps)).reshape(-1)


def _up(p, size):
    if tuple(p.shape[2:]) == tuple(size):
        return p
    return F.interpolate(p, size=tuple(size), mode="trilinear", align_corners=True)


def _at_floor(p, size):
    """p at the low-resolution cell floor(src) of every output voxel (align_corners=True)."""
    for ax, n_out in zip((2, 3, 4), size):
        n_in = p.shape[ax]
        src = torch.arange(n_out, dtype=torch.float64) * ((n_in - 1) / max(n_out - 1, 1))
        p = p.index_select(ax, src.floor().long().clamp(max=n_in - 1))
    return p


def upcat(ta, tu, wa, wu):
    """1x1x1 conv over cat(ta, up(tu)) as Wa.ta + up(Wu.tu) -> (out, mags); mags: ``a`` of Wa.ta,
    ``p`` = up(|Wu.tu|) (|p| at the eight corners), ``pm`` = up(|Wu|.|tu|), ``range`` = per axis the
    largest step |p[i+1] - p[i]| along it within the 3x3x3 low-resolution cells around floor(src)
    (the corners of the exact and of a slightly displaced source coordinate), ``n`` = p's size."""
    size = ta.shape[2:]
    ra, ma = pointwise(ta, wa)
    p, pm = pointwise(tu, wu)
    step = [torch.cat((p.diff(dim=ax).abs(), torch.zeros_like(p.narrow(ax, 0, 1))), ax) for ax in (2, 3, 4)]
    spread = [_at_floor(F.max_pool3d(s, 3, 1, 1), size) for s in step]
    return ra + _up(p, size), dict(a=ma, p=_up(p.abs(), size), pm=_up(pm, size), range=spread, n=tuple(p.shape[2:]))


def normals(mde, gain):
    return R.estimate_normals(np.asarray(mde, np.float32), gain)


def masked_volume(n2, n3, m2, m3, nbins=8):
    """The masked one-hot mono volume of the oracle (stereoanywhere.py:136, :161) as
    [B, nbins, W2, H, W1] float32, and its 0/1 cell mask (both pixels in the bin)."""
    ml, mr = R.generate_masks(m2, nbins), R.generate_masks(m3, nbins)
    vol = R.masked_mono_volume(R.mono_corr_volume(n2, n3), ml, mr)
    hit = R.masked_mono_volume(np.ones(vol.shape[:1] + vol.shape[2:], np.float32), ml, mr)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(0, 1, 4, 2, 3)))
    return to(vol), to(hit)

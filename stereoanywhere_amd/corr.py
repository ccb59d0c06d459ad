"""HIP implementation of the reference's correlation plug-in point.

Reference contract (models/stereoanywhere/corr.py):
  * ``CorrBlock1D.corr(fmap2 [B,C,H,W1], fmap3 [B,C,H,W2]) -> [B,H,W1,1,W2]`` (117-132)
  * ``CorrBlock1D(fullcorr, num_levels=4, radius=4, pad=[0,0])`` builds the pyramid (76-91)
  * ``block(coords [B,2,H,W]) -> [B, num_levels*(2r+1), H, W - pad0 - pad1]`` (93-115)
selected by ``args.corr_implementation`` (stereoanywhere.py:25, 128-133).

``HipCorrBlock1D`` keeps that contract; the pyramid lives in one buffer with the levels
of a pixel row back to back (include/stereoanywhere_hip.h) and ``corr_pyramid`` exposes
per-level views shaped like the reference's.  ``HipCorrBlock1D.from_features`` is the
fused entry (volume + truncation + pyramid in one kernel) the model uses.

The three contract methods are differentiable (csrc/corr_backward.hip): with grad mode on and an
input that requires grad they run as the autograd functions below, otherwise they make the plain
``ops`` calls of the inference path and return tensors without a ``grad_fn``.  Coordinates get no
gradient; ``__call__`` raises on coordinates that require grad.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch.autograd.function import once_differentiable

from . import ops


def _wants_grad(*tensors) -> bool:
    """Grad mode is on and one of the tensors requires grad: the autograd functions below are
    used; otherwise the contract methods make the plain ``ops`` calls of the inference path."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class _CorrVolumeFn(torch.autograd.Function):
    """ops.corr_volume with ops.corr_volume_backward as its adjoint (double backward is not built)."""

    @staticmethod
    def forward(ctx, fmap2, fmap3):
        ctx.save_for_backward(fmap2, fmap3)
        return ops.corr_volume(fmap2, fmap3)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        fmap2, fmap3 = ctx.saved_tensors
        need2, need3 = ctx.needs_input_grad
        if not (need2 or need3):
            return None, None
        return ops.corr_volume_backward(grad.contiguous(), fmap2, fmap3, need2, need3)


class _PyramidFn(torch.autograd.Function):
    """ops.pyramid_from_volume of a [rows, W2] volume with ops.pyramid_backward as its adjoint."""

    @staticmethod
    def forward(ctx, volume, num_levels):
        ctx.geo = (volume.shape[-1], num_levels)
        return ops.pyramid_from_volume(volume, num_levels)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        W2, num_levels = ctx.geo
        return ops.pyramid_backward(grad.contiguous(), W2, num_levels), None


class _LookupFn(torch.autograd.Function):
    """ops.corr_lookup of one pyramid with ops.corr_lookup_backward as its adjoint with respect to
    the pyramid buffer.  The coordinates get no gradient (the caller has checked that they ask
    for none): the reference detaches them at the top of every iteration (stereoanywhere.py:268)."""

    @staticmethod
    def forward(ctx, pyramid, coords_x, W2, num_levels, radius):
        ctx.save_for_backward(coords_x)
        ctx.geo = (W2, num_levels, radius, pyramid.shape[1])
        return ops.corr_lookup(pyramid, None, W2, num_levels, radius, coords_x)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        coords_x, = ctx.saved_tensors
        W2, num_levels, radius, rs = ctx.geo
        return ops.corr_lookup_backward(grad.contiguous(), coords_x, W2, num_levels, radius, rs), None, None, None, None


class HipCorrBlock1D:
    def __init__(self, fullcorr: Optional[torch.Tensor], num_levels: int = 4, radius: int = 4,
                 pad: Sequence[int] = (0, 0), _pyramid: Optional[torch.Tensor] = None,
                 _shape: Optional[tuple] = None):
        self.num_levels = num_levels
        self.radius = radius
        self.pad = list(pad)
        if _pyramid is None and fullcorr is None:
            if _shape is None:
                raise RuntimeError("HipCorrBlock1D needs a volume, a pyramid or (sheared-only) a shape")
        elif _pyramid is None:
            if fullcorr.dim() != 5 or fullcorr.shape[3] != 1:
                raise RuntimeError(f"fullcorr must be [B,H,W1,1,W2], got {tuple(fullcorr.shape)}")
            B, H, W1, _, W2 = fullcorr.shape
            if _wants_grad(fullcorr):   # the buffer stays in the graph: every lookup's gradient sums into it
                _pyramid = _PyramidFn.apply(fullcorr.reshape(B * H * W1, W2), num_levels)
            else:
                _pyramid = ops.pyramid_from_volume(fullcorr.reshape(B * H * W1, W2), num_levels)
            _shape = (B, H, W1, W2)
        self.shape = _shape
        self.pyramid = _pyramid
        self.sheared = None   # disparity-sheared copy for the fused lookup (shear())
        self._views = None

    @property
    def corr_pyramid(self):
        """The reference's ``corr_pyramid`` list (corr.py:85-91): num_levels + 1 tensors of
        shape [B*H*W1, 1, 1, W2 >> i].  Levels 0..num_levels-1 are views of the lookup's
        buffer; the last level, which the reference builds and never reads, is pooled from
        the one before it on first access (one HIP pyramid launch), not in the forward."""
        if self._views is None:
            B, H, W1, W2 = self.shape
            _, offs, wids = ops.pyramid_geometry(W2, self.num_levels)
            views = [self.pyramid[:, o:o + w].unsqueeze(1).unsqueeze(1) for o, w in zip(offs, wids)]
            last = views[-1].reshape(-1, wids[-1])
            if wids[-1] >= 2:
                if _wants_grad(last):
                    extra = _PyramidFn.apply(last.contiguous(), 2)
                else:
                    extra = ops.pyramid_from_volume(last.contiguous(), 2)
                w = wids[-1] // 2
                views.append(extra[:, wids[-1]:wids[-1] + w].unsqueeze(1).unsqueeze(1))
            else:   # avg_pool2d of a width-1 (or 0) row is empty
                views.append(last.new_empty((last.shape[0], 1, 1, 0)))
            self._views = views
        return self._views

    @classmethod
    def from_features(cls, fmap2: torch.Tensor, fmap3: torch.Tensor, num_levels: int = 4, radius: int = 4,
                      trunc_disp: Optional[torch.Tensor] = None, trunc_conf: Optional[torch.Tensor] = None,
                      attenuation: float = 0.9, pad: Sequence[int] = (0, 0),
                      sheared: bool = False) -> "HipCorrBlock1D":
        """corr -> x truncation volume -> pyramid fused (stereoanywhere.py:135, 201-205, 253-255).
        sheared: write the disparity-sheared layout only (ops.corr_volume_pyramid_sheared; the
        row layout where that kernel does not apply)."""
        B, _, H, W1 = fmap2.shape
        W2 = fmap3.shape[3]
        if sheared:
            sh = ops.corr_volume_pyramid_sheared(fmap2, fmap3, num_levels, trunc_disp, trunc_conf, attenuation)
            if sh is not None:
                blk = cls(None, num_levels, radius, pad, _shape=(B, H, W1, W2))
                blk.sheared = sh
                return blk
        pyr = ops.corr_volume_pyramid(fmap2, fmap3, num_levels, trunc_disp, trunc_conf, attenuation)
        return cls(None, num_levels, radius, pad, _pyramid=pyr, _shape=(B, H, W1, W2))

    def lookup_into(self, coords_x: torch.Tensor, out: torch.Tensor, other: Optional["HipCorrBlock1D"] = None):
        """Look up this pyramid (and ``other``'s, same geometry) at coords_x [B,1,H,W1] into
        out [B, nvol*L*(2r+1), H, W1] — one launch for both volumes."""
        ops.corr_lookup(self.pyramid, None if other is None else other.pyramid, self.shape[3], self.num_levels,
                        self.radius, coords_x, out)
        return out

    def shear(self, release: bool = False) -> "HipCorrBlock1D":
        """Build the disparity-sheared copy the fused lookup reads (ops.corr_pyramid_shear);
        release: drop the row-layout buffer afterwards (the per-level views need it)."""
        B, H, W1, W2 = self.shape
        self.sheared = ops.corr_pyramid_shear(self.pyramid, B, H, W1, W2, self.num_levels)
        if release:
            self.pyramid, self._views = None, None
        return self

    def lookup_conv1x1_into(self, coords_x: torch.Tensor, weight_kc: torch.Tensor, bias: torch.Tensor,
                            out: torch.Tensor, other: Optional["HipCorrBlock1D"] = None):
        """Lookup of this pyramid (and ``other``'s) followed, in the same kernel, by a 1x1 conv
        + bias + ReLU of the taps -> out [B*nvol, Cout, H, W1] (sample b*nvol + v); on the
        sheared copies when both blocks have one.  num_levels 1..4, radius 1..8, Cout 64."""
        if self.sheared is not None and (other is None or other.sheared is not None):
            return ops.corr_lookup_conv1x1_sheared(self.sheared, None if other is None else other.sheared,
                                                   self.shape[3], self.num_levels, self.radius, coords_x, weight_kc,
                                                   bias, out)
        return ops.corr_lookup_conv1x1(self.pyramid, None if other is None else other.pyramid, self.shape[3],
                                       self.num_levels, self.radius, coords_x, weight_kc, bias, out)

    def __call__(self, coords: torch.Tensor) -> torch.Tensor:
        if torch.is_grad_enabled() and coords.requires_grad:
            raise RuntimeError("HipCorrBlock1D: the lookup has no gradient with respect to the coordinates; "
                               "detach the coordinates first (coords.detach(), as the reference does at the top "
                               "of every iteration)")
        x = coords[:, :1]
        if self.pad[0]:
            x = x + self.pad[0]
        if not x.is_contiguous() and x.stride(3) != 1:
            x = x.contiguous()
        if _wants_grad(self.pyramid):
            out = _LookupFn.apply(self.pyramid, x, self.shape[3], self.num_levels, self.radius)
        else:
            out = ops.corr_lookup(self.pyramid, None, self.shape[3], self.num_levels, self.radius, x)
        W1 = out.shape[-1]
        if self.pad[0] or self.pad[1]:
            out = out[..., self.pad[0]:W1 - self.pad[1]].contiguous()
        return out

    @staticmethod
    def corr(fmap2: torch.Tensor, fmap3: torch.Tensor) -> torch.Tensor:
        fmap2, fmap3 = fmap2.float().contiguous(), fmap3.float().contiguous()
        if _wants_grad(fmap2, fmap3):
            return _CorrVolumeFn.apply(fmap2, fmap3)
        return ops.corr_volume(fmap2, fmap3)


class CorrSampler(torch.autograd.Function):
    """Replacement of the reference's native-sampler hook (corr.py:17-29,
    ``corr_sampler.forward(volume [B,H,W1,W_i], coords [B,1,H,W1], radius)`` -> the 2r+1 taps
    of one pyramid level at x = coords, linear interpolation, zero outside [0, W_i - 1]).
    One HIP lookup over a one-level pyramid; backward returns the volume's gradient (the lookup's
    and the pyramid's adjoints at one level) and, as RAFT's ``corr_sampler.backward``, none for the
    coordinates.  Double backward is not built."""

    @staticmethod
    def forward(ctx, volume, coords, radius):
        B, H, W1, Wi = volume.shape
        pyr = ops.pyramid_from_volume(volume.contiguous().reshape(B * H * W1, Wi), 1)
        x = coords[:, :1].contiguous()
        ctx.save_for_backward(x)
        ctx.geo = (tuple(volume.shape), int(radius), pyr.shape[1])
        return ops.corr_lookup(pyr, None, Wi, 1, int(radius), x)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        x, = ctx.saved_tensors
        shape, radius, rs = ctx.geo
        grad_pyr = ops.corr_lookup_backward(grad_output.contiguous(), x, shape[3], 1, radius, rs)
        return ops.pyramid_backward(grad_pyr, shape[3], 1).view(shape), None, None


# args.corr_implementation -> block class.  The reference's "reg" (torch) and "reg_cuda"
# (unvendored RAFT sampler, broken at corr.py:56) both resolve to the HIP block: this
# package IS the replacement of that plug-in point, and it has no CPU fallback.
CORR_IMPLEMENTATIONS = {"hip": HipCorrBlock1D, "reg": HipCorrBlock1D, "reg_cuda": HipCorrBlock1D}


def get_corr_block(name: str):
    try:
        return CORR_IMPLEMENTATIONS[name]
    except KeyError:
        raise NotImplementedError(f"corr_implementation={name!r}") from None

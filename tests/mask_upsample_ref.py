"""Float64 reference of sa_mask_upsample and its per-output error bound (see
tests/test_gpu_mask_upsample.py for the derivation), shared by the operator and the model tests."""
import math

import torch
import torch.nn.functional as F


def reference(x, w, b, scale, flow):
    """(ref [B,1,4H,4W] float64, bound [B,1,4H,4W] float64) from the fp32 inputs."""
    B, _, H, W = x.shape
    z = (F.conv2d(x.double(), w.double(), b.double()) * scale).view(B, 9, 4, 4, H, W)
    eps = 2e-6 * float(z.abs().max())
    nb = F.unfold(4 * flow.double(), [3, 3], padding=1).view(B, 9, 1, 1, H, W)   # zero padding
    up = (torch.softmax(z, dim=1) * nb).sum(1)                                  # [B, 4, 4, H, W]
    ref = up.permute(0, 3, 1, 4, 2).reshape(B, 1, 4 * H, 4 * W)
    R = (nb.amax(1) - nb.amin(1)).expand(B, 4, 4, H, W)
    M = nb.abs().amax(1).expand(B, 4, 4, H, W)
    bound = math.expm1(2 * eps) * R + 64 * 2.0 ** -24 * M
    return ref, bound.permute(0, 3, 1, 4, 2).reshape(B, 1, 4 * H, 4 * W)

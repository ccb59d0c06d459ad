// The coordinate / tap arithmetic of softLRC's disparity warp (utils.py:172-198), shared by the
// forward (lsq.hip) and its adjoint (lsq_backward.hip): the backward recomputes the forward's floor,
// weights and bounds from these functions, so both sides pick the same taps.
#pragma once

#include "sa_common.h"

namespace sa {

__device__ __forceinline__ float softplus_ref(float x) {
  // torch softplus(beta=1, threshold=20)
  return x > 20.0f ? x : log1pf(expf(x));
}

// The 2x2 taps of grid_sample(bilinear, zeros, align_corners=True) on an [H,W] plane at the grid point
// (gx, gy) already normalised to [-1, 1] (ATen CPU ApplyGridSample order): rows yi, yi + 1 with
// weights s, n and columns xi, xi + 1 with weights e, w (nw = s e, ne = s w, sw = n e, se = n w); a
// tap outside the plane contributes 0.
struct LrcTaps {
  int xi, yi;
  float w, e, n, s;
  float nw, ne, sw, se;
};

__device__ __forceinline__ LrcTaps lrc_taps(int H, int W, float gx, float gy) {
  const float ix = (gx + 1.0f) * ((float)(W - 1) / 2.0f);
  const float iy = (gy + 1.0f) * ((float)(H - 1) / 2.0f);
  float xw = floorf(ix), yn = floorf(iy);
  const float w = ix - xw, e = 1.0f - w;
  const float n = iy - yn, s = 1.0f - n;
  const float nw = s * e, ne = s * w, sw = n * e, se = n * w;
  xw = fminf(fmaxf(xw, -2.0f), (float)W + 1.0f);
  yn = fminf(fmaxf(yn, -2.0f), (float)H + 1.0f);
  const int xi = (int)xw, yi = (int)yn;
  return LrcTaps{xi, yi, w, e, n, s, nw, ne, sw, se};
}

__device__ __forceinline__ bool lrc_inside(int H, int W, int y, int x) {
  return x >= 0 && x <= W - 1 && y >= 0 && y <= H - 1;
}

// The grid point pixel (y, x) samples the other map at, given its own relu'd disparity dsrc.
// sign = -1: left map (x - dsrc), +1: right map (x + dsrc).  Normalised by W and H under
// align_corners=True (the reference's quirk): ix = (x -+ dsrc) (W - 1) / W, iy = y (H - 1) / H.
__device__ __forceinline__ void lrc_grid(int H, int W, int y, int x, float dsrc, float sign, float &gx, float &gy) {
  const float xn = sign < 0 ? ((float)x - dsrc) : ((float)x + dsrc);
  gx = 2.0f * (xn / (float)W) - 1.0f;
  gy = 2.0f * ((float)y / (float)H) - 1.0f;
}

}  // namespace sa

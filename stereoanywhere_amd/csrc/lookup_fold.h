// Lookup + convc1 for any pyramid geometry (1..4 levels, radius 1..8), shared by the row-layout
// (corr_lookup.hip) and the disparity-sheared (corr_shear.hip) kernels, so that both layouts
// give the same bits from the same cells.
//
// One thread per (volume, pixel).  The taps are produced level by level, t ascending, and each is
// folded at once into the thread's COUT fp32 accumulators as a rank-1 update with wave-uniform
// weights (scalar loads): no tap array, so L and R are run-time values and the register
// count does not depend on them.
//   tap: the fp32 expressions of lookup_kernel (corr_lookup.hip): grid round trip, floor,
//        zero outside [0, W_l - 1], v0 * (1 - w) + v1 * w
//   conv: acc[c] = bias[c]; acc[c] = fmaf(w[k][c], tap[k], acc[c]) for k = l * (2R + 1) + t + R
//        ascending; ReLU by the caller: the chain of the (4, 4) kernels
#pragma once

namespace sa {

// cell(l, k): value of level l's cell k of this thread's pixel; called only for k in [0, W_l - 1]
template <int COUT, class Cell>
__device__ __forceinline__ void lookup_c1_fold(float x, int L, int R, const int (&wid)[4],
                                               const float *__restrict__ wt, const float *__restrict__ bias,
                                               Cell cell, float (&acc)[COUT]) {
#pragma unroll
  for (int c = 0; c < COUT; ++c) acc[c] = bias[c];
  const float *__restrict__ wk = wt;   // row k of weight_kc, k ascending with the taps
  for (int l = 0; l < L; ++l) {
    const int Wl = wid[l];
    const float xl = x / (float)(1 << l);
    const float denom = (float)(Wl - 1);
    const float sf = (float)(Wl - 1) / 2.0f;
    for (int t = -R; t <= R; ++t) {
      const float x0 = (float)t + xl;
      const float xg = 2.0f * x0 / denom - 1.0f;
      const float ix = (xg + 1.0f) * sf;
      float xw = floorf(ix);
      const float w = ix - xw;
      const float e = 1.0f - w;
      xw = fminf(fmaxf(xw, -2.0f), (float)Wl + 1.0f);   // keep the int conversion defined
      const int xi = (int)xw;
      const float v0 = (xi >= 0 && xi <= Wl - 1) ? cell(l, xi) : 0.0f;
      const float v1 = (xi + 1 >= 0 && xi + 1 <= Wl - 1) ? cell(l, xi + 1) : 0.0f;
      const float tap = v0 * e + v1 * w;
#pragma unroll
      for (int c = 0; c < COUT; ++c) acc[c] = fmaf(wk[c], tap, acc[c]);
      wk += COUT;
    }
  }
}

}  // namespace sa

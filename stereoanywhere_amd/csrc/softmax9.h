// The nine-tap softmax and convex combination of convex_upflow (utils.py:97-110) for upsample.hip,
// mask_upsample.hip and diffops_backward.hip: the outputs that the tests compare bit for bit come
// from the same operations in the same order.
#pragma once

#include "sa_common.h"

namespace sa {

// lg -> softmax(lg) in place: max, exp, sum, reciprocal, then each weight times the reciprocal
__device__ __forceinline__ void softmax9(float (&lg)[9]) {
  float mx = -INFINITY, s = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) mx = fmaxf(mx, lg[k]);
#pragma unroll
  for (int k = 0; k < 9; ++k) s += lg[k] = expf(lg[k] - mx);
  const float inv = 1.0f / s;
#pragma unroll
  for (int k = 0; k < 9; ++k) lg[k] *= inv;
}

// sum_k softmax(lg)_k v_k in k order: softmax9's operations on a copy (written out: keep the two in
// step), each weight used as it is scaled
__device__ __forceinline__ float convex_px(const float (&lg_in)[9], const float (&v)[9]) {
  float lg[9], mx = -INFINITY, s = 0.f, acc = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) mx = fmaxf(mx, lg[k] = lg_in[k]);
#pragma unroll
  for (int k = 0; k < 9; ++k) s += lg[k] = expf(lg[k] - mx);
  const float inv = 1.0f / s;
#pragma unroll
  for (int k = 0; k < 9; ++k) acc += (lg[k] * inv) * v[k];
  return acc;
}

}  // namespace sa

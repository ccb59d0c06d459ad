// The arithmetic of the kernels that multiply fp32 values as f16 hi / lo pairs on v_mfma_f32_16x16x32_f16
// (conv1x1, mask_upsample, conv3d_mfma, conv3d_s2mf), defined once so that kernels which must agree bit
// for bit run the same operations.  v = hi + lo exactly in fp32 (22 significant bits); w * x = hi hi +
// hi lo + lo hi, accumulated in fp32 in that order per 32 k (the lo lo term is below 2^-22 of the product).
// This header holds no multiply-add (conversions, one subtraction, one sum times a constant, MFMA
// builtins): it compiles the same with `#pragma clang fp contract(fast)` as without.
#pragma once

#include "sa_common.h"

namespace sa {

constexpr float kSplitScale = 4096.0f;   // 2^12 on the weights before the split: their lo halves stay normal f16
constexpr float kF16Max = 65504.0f;      // from here on a value's hi half is infinite (the range guards)

__device__ __forceinline__ void split_f16(float v, _Float16 &hi, _Float16 &lo) {
  hi = (_Float16)v;                  // round to nearest even
  lo = (_Float16)(v - (float)hi);    // (the difference is exact in fp32)
}

// ... of an input that may leave the f16 range: true for |v| >= kF16Max or NaN, for the caller to OR into
// its block's flag
__device__ __forceinline__ bool split_f16_guarded(float v, _Float16 &hi, _Float16 &lo) {
  split_f16(v, hi, lo);
  return !(__builtin_fabsf(v) < kF16Max);
}

// ... of one MFMA operand's 8 consecutive k; `bad` goes in and comes back by value
__device__ __forceinline__ bool split_f16x8_guarded(const float (&v)[8], f16x8 &hi, f16x8 &lo, bool bad) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    _Float16 h, l;
    const bool o = split_f16_guarded(v[j], h, l);
    hi[j] = h;
    lo[j] = l;
    bad |= o;
  }
  return bad;
}

// One accumulator's three products of a 32-k step, A = (ah, al), B = (bh, bl)
__device__ __forceinline__ void mfma_split3(f32x4 &acc, f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);
}

// The same for MT x NT accumulators, product-major: an accumulator's products are MT x NT MFMAs apart
template <int MT, int NT>
__device__ __forceinline__ void mfma_split3_tile(f32x4 (&acc)[MT][NT], const f16x8 (&ah)[MT], const f16x8 (&al)[MT],
                                                 const f16x8 (&bh)[NT], const f16x8 (&bl)[NT]) {
#pragma unroll
  for (int p = 0; p < 3; ++p)   // hi hi, hi lo, lo hi
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int n = 0; n < NT; ++n)
        acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(p < 2 ? ah[t] : al[t], p == 1 ? bl[n] : bh[n], acc[t][n], 0, 0, 0);
}

// the fp32 weight a range guard's redo pass rebuilds from a pre-split pair
__device__ __forceinline__ float split_weight_f32(_Float16 hi, _Float16 lo) {
  return ((float)hi + (float)lo) * (1.0f / kSplitScale);
}

}  // namespace sa

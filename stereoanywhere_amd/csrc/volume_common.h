// Per-cell device functions shared by the kernels that read or write cost volumes: the depth bin of
// a mono value (mono_volume.hip, volume_stage.hip) and the analytic truncation factor (the epilogues
// of corr_volume.hip, volume_stage.hip).  One definition each, so the producers and the stand-alone
// stage cannot drift apart.
#pragma once

#include "sa_common.h"

namespace sa {

// generate_masks (utils.py:48-54): bin n holds n/N <= m < (n+1)/N, so 1.0, negative values and NaN
// are in no bin (-1).
__device__ __forceinline__ int depth_bin(float m, int nbins) {
  // m*nbins is exact for power-of-two nbins; the general case compares like the reference
  for (int n = 0; n < nbins; ++n) {
    if (m < (float)(n + 1) / (float)nbins && m >= (float)n / (float)nbins) return n;
  }
  return -1;
}

// truncate_corr_volume_v2 (utils.py:216-238) for cell (j, k) of a left pixel with disparity d and
// confidence m: 1 (1 - m) + m (sigmoid((j - d) - k) (1 - atten) + atten), the reference's operations
// in its order.  FAST: the hardware-exp2 sigmoid (sigmoidf_fast) in place of 1 / (1 + expf(-x)).
template <bool FAST>
__device__ __forceinline__ float trunc_factor(int j, int k, float d, float m, float atten) {
  const float center = (float)j - d;
  const float tv = center - (float)k;
  const float s = FAST ? sigmoidf_fast(tv) : sigmoidf_ref(tv);
  return 1.0f * (1.0f - m) + m * (s * (1.0f - atten) + atten);
}

}  // namespace sa

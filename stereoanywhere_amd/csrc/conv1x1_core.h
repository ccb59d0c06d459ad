// The all-channel 1x1 GEMM core of conv1x1_v2_kernel (conv1x1.hip) and mask_upsample_kernel
// (mask_upsample.hip): a block's PX pixels staged once as f16 hi / lo planes [k / 8][pixel][8] (a lane's
// B operand is one 16-byte LDS read), a wave's MT channel tiles against NT = PX / 16 pixel tiles, the A
// operands (pre-split weights [Cout][Cin], hi and lo planes) from global memory two 32-k steps ahead.
// Both kernels run these functions: the same logit bits; grids, pass loops, LDS sizing, stores, redo passes stay
// theirs.  Lane roles: am = lane % 16 (A: channel row, B: pixel of a tile), aq = lane / 16 (k = 8 aq .. + 7 of 32).
#pragma once

#include "split_f16.h"

namespace sa {

// staging: one thread's 8 consecutive k (group kg) of pixel px, split into both planes
template <int PX>
__device__ __forceinline__ bool c1_stage8(const float (&v)[8], _Float16 *xh, _Float16 *xl, int kg, int px, bool bad) {
  f16x8 h, l;
  bad = split_f16x8_guarded(v, h, l, bad);
  *reinterpret_cast<f16x8 *>(&xh[(kg * PX + px) * 8]) = h;
  *reinterpret_cast<f16x8 *>(&xl[(kg * PX + px) * 8]) = l;
  return bad;
}

// A wave's walk over the weights: its first channel tile t0 and `total` steps (passes x NKS), the last
// weight row (read with PASSES only), and the lane roles
struct C1Wave { int t0, total, rowmax, am, aq; };

// A operands of step `it` of the wave's `total` (pass it / NKS, 32-k step it % NKS; clamped: the loads
// past the last step are unconditional, never used): the pass's MT channel tiles from tile t0 on.
// PASSES: several passes, the last tile may be ragged (a wave-uniform run-time step, rows held at rowmax);
// else one pass of whole tiles.
template <int MT, int NKS, bool PASSES>
__device__ __forceinline__ void c1_load_w(const _Float16 *whi, const _Float16 *wlo, const C1Wave &w, int Cin, int it, f16x8 (&wh)[MT], f16x8 (&wl)[MT]) {
  it = min(it, max(w.total - 1, 0));
  if (PASSES) it = __builtin_amdgcn_readfirstlane(it);
  const int ps = it / NKS, ks = it - ps * NKS;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int row = 16 * (w.t0 + ps * MT + t) + w.am;
    const long o = (long)(PASSES ? min(row, w.rowmax) : row) * Cin + ks * 32 + w.aq * 8;
    wh[t] = *reinterpret_cast<const f16x8 *>(whi + o);
    wl[t] = *reinterpret_cast<const f16x8 *>(wlo + o);
  }
}

// Step `it`: the tile's MFMAs on (wh, wl), then that register set's loads for step it + 2 (the next set is
// in flight).  (Unbarred, the scheduler sinks a step's loads past the next step's MFMAs: both sets wait together.)
template <int PX, int MT, int NT, int NKS, bool PASSES>
__device__ __forceinline__ void c1_step(f32x4 (&acc)[MT][NT], const _Float16 *xh, const _Float16 *xl, const _Float16 *whi,
                                        const _Float16 *wlo, const C1Wave &w,
                                        int Cin, int it, f16x8 (&wh)[MT], f16x8 (&wl)[MT]) {
  const int kg = (it % NKS) * 4 + w.aq;
  f16x8 bh[NT], bl[NT];   // B operands of k-group kg for the NT pixel tiles
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    bh[n] = *reinterpret_cast<const f16x8 *>(&xh[(kg * PX + 16 * n + w.am) * 8]);
    bl[n] = *reinterpret_cast<const f16x8 *>(&xl[(kg * PX + 16 * n + w.am) * 8]);
  }
  mfma_split3_tile<MT, NT>(acc, wh, wl, bh, bl);
  c1_load_w<MT, NKS, PASSES>(whi, wlo, w, Cin, it + 2, wh, wl);
  __builtin_amdgcn_sched_barrier(0);
}

}  // namespace sa

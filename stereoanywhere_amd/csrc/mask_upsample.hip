// The mask head's 1x1 conv (update.py:159-162, 191: 256 -> 9 * 16 logits, x 0.25), the softmax over
// the nine neighbours and the convex up-sampling (convex_upflow, utils.py:97-110, factor 4) in one
// kernel: the full-outputs forward runs this once per GRU iteration, and the [B, 144, H, W] logit
// tensor that sa_conv1x1 would write and sa_convex_upsample read back stays in LDS.
//
//   out[b][4 h + a][4 w + c] = sum_k softmax_k(z[b][16 k + 4 a + c][h][w]) * 4 flow[b][h + k / 3 - 1][w + k % 3 - 1]
//   z[b][co][p] = scale * (bias[co] + sum_ci W[co][ci] x[b][ci][p])        (flow zero-padded)
//
// Products as in conv1x1.hip: the same pre-split weights, and conv1x1_core.h's functions that
// conv1x1_v2_kernel runs, so the logits are the bits sa_conv1x1 writes.  Softmax and weighted sum are
// convex_up_px_kernel's (upsample.hip): softmax9.h's convex_px.
//
//   block = 3 waves, 48 consecutive pixels of one image's flat H*W plane (pixels past the plane's
//           end are staged as zeros and never stored) for all 144 channels.  The pixels' Cin inputs
//           are read once, split and kept in LDS as [k / 8][pixel][8] halves (a lane's B operand is
//           one 16-byte read).
//   wave  = 3 of the 9 channel tiles (48 channels = the 16 sub-pixels of 3 neighbours) x the 3
//           pixel tiles: 9 MFMA tiles, 36 accumulators, 27 MFMAs per 32 k against 6 KB of A
//           operands (pre-split weights, from L2).  The block reads the weights once.
//   exchange: after the last MFMA the logits go to LDS as [channel][pixel] (pitch 60 floats: the
//           accumulator writes and the reads below are conflict-free), over the staged input.
//   epilogue: thread = (pixel, sub-row a), 48 x 4 = the block's 192 threads: its 36 logits from LDS,
//           the 9 neighbours of 4 flow (loaded at the kernel's start), 4 softmaxes, one float4 of
//           output row 4 h + a (16-byte aligned whenever out and its batch stride are).
//   range guard: an input of magnitude >= 65504 (f16 overflow) makes the block compute its logits
//           with fp32 FMAs (as conv1x1_v2_kernel does) before the same epilogue.
#include "conv1x1_core.h"
#include "softmax9.h"

#include <cstdint>

namespace {

using sa::f32x4, sa::f16x8;

constexpr int MU_PX = 48, MU_THR = 192, MU_CO = 144, MU_MT = 3, MU_NT = 3;
constexpr int MU_LG_PITCH = 60;   // floats per logit row: rows 4 apart start 48 banks apart

__device__ unsigned g_mu_redo_blocks;

constexpr int mu_lds_bytes(int nks) {
  const int xb = 2 * nks * 4 * MU_PX * 8 * 2, lb = MU_CO * MU_LG_PITCH * 4;
  return xb > lb ? xb : lb;
}

template <int NKS>   // Cin / 32
__global__ __launch_bounds__(MU_THR) void mask_upsample_kernel(const float *__restrict__ x, long x_bs, int H, int W,
                                                               const _Float16 *__restrict__ whi,
                                                               const _Float16 *__restrict__ wlo,
                                                               const float *__restrict__ bias, float scale,
                                                               const float *__restrict__ flow,
                                                               float *__restrict__ out, long out_bs, long px_blocks) {
  constexpr int Cin = NKS * 32, ngrp = Cin / 8;
  constexpr int XH = ngrp * MU_PX * 8;   // halves per plane
  __shared__ __attribute__((aligned(16))) unsigned char smem[mu_lds_bytes(NKS)];
  __shared__ float bs[MU_CO];
  _Float16 *xh = reinterpret_cast<_Float16 *>(smem), *xl = xh + XH;
  float *lgs = reinterpret_cast<float *>(smem);   // [channel][MU_LG_PITCH], once the MFMAs have read xh / xl
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned lid = sa::xcd_remap(blockIdx.x, gridDim.x);
  const long P = (long)H * W;
  const long pb = lid % px_blocks;
  const int b = (int)(lid / px_blocks);
  const long p0 = pb * MU_PX;
  const float *xb = x + (long)b * x_bs;
  if (tid < MU_CO) bs[tid] = bias ? bias[tid] : 0.0f;

  // the epilogue's pixel and sub-row, and its 3x3 neighbourhood of 4 * flow (clamped loads, then the
  // zero padding as a select: no load under a branch)
  const int epx = tid % MU_PX, ea = tid / MU_PX;
  const long ep = p0 + epx;
  const bool eok = ep < P;
  const long epc = min(ep, P - 1);
  const int eh = (int)(epc / W), ew = (int)(epc % W);
  float fv[9];
  {
    const float *fl = flow + (long)b * P;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int yy = eh + k / 3 - 1, xx = ew + k % 3 - 1;
      const float t = fl[(long)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1)];
      fv[k] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? 4.0f * t : 0.0f;
    }
  }

  // staging: thread (pixel tid % 48, k-groups tid / 48 + 4 u), 8 loads per group; a pixel past the
  // plane's end loads pixel P - 1 (no load under a branch) and stages zeros
  bool bad = false;
  {
    const long pc = min(p0 + epx, P - 1);
    constexpr int NU = ngrp / 4;   // k-groups per thread: all of their loads (8 NU) in flight together
    float v[NU][8];
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) v[u][j] = xb[(long)((ea + 4 * u) * 8 + j) * P + pc];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int kg = ea + 4 * u;
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = eok ? v[u][j] : 0.0f;
      bad = sa::c1_stage8<MU_PX>(f, xh, xl, kg, epx, bad);
    }
  }
  if (__syncthreads_or(bad)) {   // range guard: the block's logits with fp32 FMAs (exact products)
    if (tid == 0) atomicAdd(&g_mu_redo_blocks, 1u);
    for (int e = tid; e < MU_CO * MU_PX; e += MU_THR) {
      const int co = e / MU_PX, px = e % MU_PX;
      const long p = p0 + px;
      float s = 0.0f;
      if (p < P)
        for (int k = 0; k < Cin; ++k) {   // (the redo dot product, as in conv1x1.hip's two kernels)
          const float w = sa::split_weight_f32(whi[(long)co * Cin + k], wlo[(long)co * Cin + k]);
          s = fmaf(w, xb[(long)k * P + p], s);
        }
      lgs[co * MU_LG_PITCH + px] = (s + bs[co]) * scale;
    }
  } else {
    const int am = lane & 15, aq = lane >> 4;   // A: channel row am of a tile, k = 8 aq .. + 7; B: pixel am of a tile
    const int t0 = __builtin_amdgcn_readfirstlane(wv) * MU_MT;
    f32x4 acc[MU_MT][MU_NT];
#pragma unroll
    for (int t = 0; t < MU_MT; ++t)
#pragma unroll
      for (int n = 0; n < MU_NT; ++n) acc[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    // conv1x1_v2_kernel's pipeline: one pass of NKS steps, every tile whole
    const sa::C1Wave wave{t0, NKS, MU_CO - 1, am, aq};
    auto step = [&](int ks, f16x8 (&wh)[MU_MT], f16x8 (&wl)[MU_MT]) __attribute__((always_inline)) {
      sa::c1_step<MU_PX, MU_MT, MU_NT, NKS, false>(acc, xh, xl, whi, wlo, wave, Cin, ks, wh, wl);
    };
    f16x8 wha[MU_MT], wla[MU_MT], whb[MU_MT], wlb[MU_MT];
    sa::c1_load_w<MU_MT, NKS, false>(whi, wlo, wave, Cin, 0, wha, wla);
    sa::c1_load_w<MU_MT, NKS, false>(whi, wlo, wave, Cin, 1, whb, wlb);
#pragma unroll
    for (int ks = 0; ks < NKS; ks += 2) {   // (NKS even: Cin 64, 128, 256)
      step(ks, wha, wla);
      step(ks + 1, whb, wlb);
    }
    __syncthreads();   // every wave has read its last B operands: the logits go over xh / xl
    // D: lane holds channels 16 tile + 4 aq + i (rows), pixel 16 n + am (column)
#pragma unroll
    for (int t = 0; t < MU_MT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int co = 16 * (t0 + t) + 4 * aq + i;
        const float bv = bs[co];
#pragma unroll
        for (int n = 0; n < MU_NT; ++n)
          lgs[co * MU_LG_PITCH + 16 * n + am] = (acc[t][n][i] * (1.0f / sa::kSplitScale) + bv) * scale;
      }
  }
  __syncthreads();
  // epilogue: channel 16 k + 4 a + c of pixel epx
  float4 o;
  float lg[4][9];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int k = 0; k < 9; ++k) lg[c][k] = lgs[(16 * k + 4 * ea + c) * MU_LG_PITCH + epx];
  o.x = sa::convex_px(lg[0], fv);
  o.y = sa::convex_px(lg[1], fv);
  o.z = sa::convex_px(lg[2], fv);
  o.w = sa::convex_px(lg[3], fv);
  if (eok) *reinterpret_cast<float4 *>(out + (long)b * out_bs + (long)(4 * eh + ea) * (4L * W) + 4 * ew) = o;
}

}  // namespace

extern "C" int sa_mask_upsample(const float *x, long x_bs, int B, int Cin, int H, int W, const void *wsplit,
                                const float *bias, float scale, const float *flow, float *out, long out_bs,
                                void *stream) {
  SA_REQUIRE(x && wsplit && flow && out, "sa_mask_upsample: null pointer");
  SA_REQUIRE(B > 0 && H > 0 && W > 0, "sa_mask_upsample: empty shape");
  SA_REQUIRE(Cin == 64 || Cin == 128 || Cin == 256, "sa_mask_upsample: Cin must be 64, 128 or 256");
  const long P = (long)H * W;
  SA_REQUIRE(P < (1L << 31) / 16, "sa_mask_upsample: plane too large");
  SA_REQUIRE(x_bs >= (long)Cin * P && out_bs >= 16 * P, "sa_mask_upsample: batch stride below the planes");
  SA_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0 && out_bs % 4 == 0,
             "sa_mask_upsample: out and its batch stride must be 16-byte granular");
  SA_REQUIRE((reinterpret_cast<uintptr_t>(wsplit) & 15) == 0, "sa_mask_upsample: weights not 16-byte aligned");
  const long px_blocks = (P + MU_PX - 1) / MU_PX;
  SA_REQUIRE(px_blocks * B < (1L << 31), "sa_mask_upsample: too many blocks");
  const _Float16 *hi = static_cast<const _Float16 *>(wsplit);
  const _Float16 *lo = hi + (long)MU_CO * Cin;
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  const unsigned g = (unsigned)(px_blocks * B);
#define SA_MU_LAUNCH(NKS) \
  mask_upsample_kernel<NKS><<<g, MU_THR, 0, s>>>(x, x_bs, H, W, hi, lo, bias, scale, flow, out, out_bs, px_blocks)
  if (Cin == 64) SA_MU_LAUNCH(2);
  else if (Cin == 128) SA_MU_LAUNCH(4);
  else SA_MU_LAUNCH(8);
#undef SA_MU_LAUNCH
  return sa::check_launch("sa_mask_upsample");
}

extern "C" long sa_mask_upsample_redo_blocks(int reset) {
  return sa::read_redo_counter(g_mu_redo_blocks, reset);
}

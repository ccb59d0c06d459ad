// Backward of the hourglass's up-cat joins (hourglass.py:319-321, 326-328): the 1x1x1 conv over
// cat(a, trilinear_up(u)) that sa_conv3d_pointwise + sa_conv3d_pointwise_upcat (conv3d_fused.hip)
// evaluate as out = Wa . a + up(p), p = Wu . u.  With g = dL/dout:
//   dp = up^T(g)                    sa_trilinear_up_adjoint
//   da = Wa^T . g,  dWa = sum a g   sa_conv3d_pointwise_backward(a, g, w_a)
//   du = Wu^T . dp, dWu = sum u dp  sa_conv3d_pointwise_backward(u, dp, w_u)
// so neither the up-sampled nor the concatenated volume, nor a gradient of either, ever exists.
//
// Volumes are [B, C, D, H, W] fp32, contiguous; weights [Cx][Cg] as the forward takes them.
//
//   up_adjoint_kernel   a gather: one wave owns UP_DZ x UP_HY low-resolution rows of one (b, c) and
//                       streams their high-resolution footprint of g as rows along W, a lane's 16 bytes at
//                       dword alignment (a row of a volume with W % 4 != 0 does not start on a 16-byte
//                       boundary).  Per chunk of 256 columns a lane folds the D and H taps of its four
//                       columns (d ascending, h ascending within), the folded rows go to LDS and lane wx
//                       sums its W taps, ascending.  The taps and weights are the forward's own fp32
//                       expressions (conv3d_fused.hip, pointwise_upcat_kernel): i = (int)(s * (float)dst),
//                       frac = s * dst - i, the +1 corner clamped onto i at the last cell; a low index's
//                       destination range is found by bisection on that (monotone) expression, so no tap
//                       count is assumed: Dp = 1 puts every plane into one cell.
//   pw_bwd_kernel       one pass over x and g: a block of 4 waves takes PW_SPAN cells of one batch
//                       sample, lanes along the cells.  A wave owns RX = Cx / S rows of x (its slice) and
//                       one of G = 4 / S interleaved groups of 64-cell steps: dx = W . g for its rows, and
//                       RX x Cg sums of x g per lane in fp32 for PW_CHAIN steps, then transposed through
//                       LDS and added into float64 (lane k < 32 adds the 64 lanes' values of sum 32 r + k
//                       in lane order).  Each wave writes its float64 partials to `work`.
//   pw_fold_kernel      one wave per dw element adds the partials in index order.
//
// Determinism: no atomics; every sum's order is fixed by indices.
#include "sa_common.h"

namespace {

// 16 bytes at dword alignment (global loads and stores of gfx950 need no more)
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// ------------------------------------------------------------------------------- up-sampling adjoint
constexpr int UP_DZ = 2, UP_HY = 4;   // low-resolution rows per block: UP_DZ planes x UP_HY rows
constexpr int UP_ROWS = UP_DZ * UP_HY;
constexpr int UP_CHUNK = 4 * 64;      // columns of g per round

// the smallest dst in [0, n_out] whose source index (int)(s * (float)dst) is at least v (n_out: none).
// The index is monotone in dst: the conversion, the rounded product and the truncation all are.
__device__ __forceinline__ int first_reaching(float s, int n_out, int v) {
  int lo = 0, hi = n_out;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int)(s * (float)mid) >= v) {
      hi = mid;
    } else {
      lo = mid + 1;
    }
  }
  return lo;
}

// what destination dst takes from low-resolution index z along one axis: the forward's two lerp weights,
// both on z where the +1 corner is clamped; 0 where z is neither corner (z >= n_in included)
__device__ __forceinline__ float tap_weight(float s, int n_in, int dst, int z) {
  const float r = s * (float)dst;
  const int i = (int)r;
  const float l1 = r - (float)i, l0 = 1.0f - l1;
  const int p = i < n_in - 1 ? 1 : 0;
  return (i == z ? l0 : 0.0f) + (i + p == z ? l1 : 0.0f);
}

__global__ __launch_bounds__(64) void up_adjoint_kernel(const float *__restrict__ g, int D, int H, int W, int Dp,
                                                        int Hp, int Wp, float sd, float sh, float sw, int tilesD,
                                                        int tilesH, float *__restrict__ dp) {
  __shared__ float rows[UP_ROWS][UP_CHUNK];
  const int lane = threadIdx.x;
  // neighbouring tiles share planes and rows of g: keep them on one XCD's L2
  const long id = sa::xcd_remap(blockIdx.x, gridDim.x);
  const int hy0 = (int)(id % tilesH) * UP_HY;
  const long t = id / tilesH;
  const int dz0 = (int)(t % tilesD) * UP_DZ;
  const long bc = t / tilesD;
  const int d_lo = first_reaching(sd, D, dz0 - 1), d_hi = first_reaching(sd, D, dz0 + UP_DZ);
  const int h_lo = first_reaching(sh, H, hy0 - 1), h_hi = first_reaching(sh, H, hy0 + UP_HY);
  const float *gv = g + bc * ((long)D * H * W);
  for (int x0 = 0; x0 < Wp; x0 += 64) {
    const int wx = x0 + lane;
    const bool live = wx < Wp;
    const int x1 = x0 + 63 < Wp - 1 ? x0 + 63 : Wp - 1;
    const int t_lo = first_reaching(sw, W, x0 - 1), t_hi = first_reaching(sw, W, x1 + 1);   // the tile's columns
    const int my_lo = live ? first_reaching(sw, W, wx - 1) : 0, my_hi = live ? first_reaching(sw, W, wx + 1) : 0;
    float sum[UP_ROWS];
#pragma unroll
    for (int k = 0; k < UP_ROWS; ++k) sum[k] = 0.0f;
    for (int c0 = t_lo; c0 < t_hi; c0 += UP_CHUNK) {
      const int w = c0 + 4 * lane;
      const int valid = t_hi - w >= 4 ? 4 : (t_hi - w > 0 ? t_hi - w : 0);   // t_hi <= W
      float acc[UP_ROWS][4];
#pragma unroll
      for (int k = 0; k < UP_ROWS; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] = 0.0f;
      for (int d = d_lo; d < d_hi; ++d) {
        float wd[UP_DZ];
#pragma unroll
        for (int i = 0; i < UP_DZ; ++i) wd[i] = tap_weight(sd, Dp, d, dz0 + i);
        for (int h = h_lo; h < h_hi; ++h) {
          const float *p = gv + ((long)d * H + h) * W + w;
          float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          if (valid == 4) {
            const f32x4u q = *reinterpret_cast<const f32x4u *>(p);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = q[e];
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (e < valid) v[e] = p[e];
          }
#pragma unroll
          for (int j = 0; j < UP_HY; ++j) {
            const float wh = tap_weight(sh, Hp, h, hy0 + j);
#pragma unroll
            for (int i = 0; i < UP_DZ; ++i) {
              const float wdh = wd[i] * wh;
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[i * UP_HY + j][e] = fmaf(wdh, v[e], acc[i * UP_HY + j][e]);
            }
          }
        }
      }
      __syncthreads();   // the chunk before has been read
#pragma unroll
      for (int k = 0; k < UP_ROWS; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) rows[k][4 * lane + e] = acc[k][e];
      __syncthreads();
      const int a = my_lo > c0 ? my_lo : c0, b = my_hi < c0 + UP_CHUNK ? my_hi : c0 + UP_CHUNK;
      for (int ww = a; ww < b; ++ww) {
        const float wt = tap_weight(sw, Wp, ww, wx);
#pragma unroll
        for (int k = 0; k < UP_ROWS; ++k) sum[k] = fmaf(wt, rows[k][ww - c0], sum[k]);
      }
    }
    if (live) {
#pragma unroll
      for (int i = 0; i < UP_DZ; ++i)
#pragma unroll
        for (int j = 0; j < UP_HY; ++j)
          if (dz0 + i < Dp && hy0 + j < Hp) dp[((bc * Dp + dz0 + i) * Hp + hy0 + j) * Wp + wx] = sum[i * UP_HY + j];
    }
  }
}

// ------------------------------------------------------------------------------- pointwise conv backward
constexpr int PW_WAVES = 4;
constexpr int PW_THREADS = 64 * PW_WAVES;
constexpr int PW_CHAIN = 32;        // fp32 products a lane adds before they go into float64
constexpr long PW_SPAN = 16384;     // cells of one batch sample per block

// S: slices of the Cx rows (one wave each); the block's other PW_WAVES / S waves interleave cell steps
template <int CX, int CG, int S, bool DX, bool DW>
__global__ __launch_bounds__(PW_THREADS) void pw_bwd_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                            const float *__restrict__ w, long n, int spans,
                                                            double *__restrict__ work, float *__restrict__ dx) {
  constexpr int G = PW_WAVES / S, RX = CX / S, NACC = RX * CG, NR = NACC / 32;
  constexpr int STEPS = (int)(PW_SPAN / (64 * G));
  static_assert(PW_WAVES % S == 0 && CX % S == 0 && NACC % 32 == 0 && STEPS % PW_CHAIN == 0, "slicing");
  __shared__ float tr[DW ? PW_WAVES : 1][DW ? 32 * 64 : 1];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int slice = wave % S, grp = wave / S;
  const long b = blockIdx.x / spans;
  const long c0 = (long)(blockIdx.x % spans) * PW_SPAN;
  const float *xb = x + (b * CX + slice * RX) * n;
  const float *gb = g + b * CG * n;
  float *dxb = DX ? dx + (b * CX + slice * RX) * n : nullptr;
  const float *ws = w + slice * RX * CG;
  float acc[DW ? NACC : 1];
  double tot[DW ? NR : 1];
  if (DW) {
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0f;
#pragma unroll
    for (int r = 0; r < NR; ++r) tot[r] = 0.0;
  }
#pragma unroll 1
  for (int step = 0; step < STEPS; ++step) {
    const long i = c0 + ((long)step * G + grp) * 64 + lane;
    const bool ok = i < n;
    float gv[CG];
#pragma unroll
    for (int c = 0; c < CG; ++c) gv[c] = ok ? gb[c * n + i] : 0.0f;
#pragma unroll
    for (int r = 0; r < RX; ++r) {
      if (DW) {
        const float xv = ok ? xb[r * n + i] : 0.0f;
#pragma unroll
        for (int c = 0; c < CG; ++c) acc[r * CG + c] = fmaf(xv, gv[c], acc[r * CG + c]);
      }
      if (DX) {
        float o = 0.0f;
#pragma unroll
        for (int c = 0; c < CG; ++c) o = fmaf(ws[r * CG + c], gv[c], o);
        if (ok) dxb[r * n + i] = o;
      }
    }
    if (DW && (step + 1) % PW_CHAIN == 0) {   // every wave of the block takes the same steps
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 32; ++k) {
          tr[wave][k * 64 + (lane ^ k)] = acc[32 * r + k];
          acc[32 * r + k] = 0.0f;
        }
        __syncthreads();
        if (lane < 32) {
          double s = tot[r];
#pragma unroll 8
          for (int l = 0; l < 64; ++l) s += (double)tr[wave][lane * 64 + (l ^ lane)];
          tot[r] = s;
        }
      }
    }
  }
  if (DW && lane < 32) {
    double *o = work + ((long)blockIdx.x * PW_WAVES + wave) * NACC;
#pragma unroll
    for (int r = 0; r < NR; ++r) o[32 * r + lane] = tot[r];
  }
}

// one wave per dw[cx][cg]: the nblk * G wave partials in index order, lanes strided, then the DPP tree
__global__ __launch_bounds__(64) void pw_fold_kernel(const double *__restrict__ work, long nblk, int S, int RX, int CG,
                                                     float *__restrict__ dw) {
  const int G = PW_WAVES / S, nacc = RX * CG;
  const int cx = blockIdx.x / CG, cg = blockIdx.x % CG;
  const int slice = cx / RX, k = (cx % RX) * CG + cg;
  double s = 0.0;
  for (long q = threadIdx.x; q < nblk * G; q += 64) {
    const long blk = q / G;
    const int wave = (int)(q % G) * S + slice;
    s += work[(blk * PW_WAVES + wave) * nacc + k];
  }
  s = sa::wave_sum_dpp_lane63(s);
  if (threadIdx.x == 63) dw[blockIdx.x] = (float)s;
}

// the slices of the built (Cx, Cg) pairs: 64 or 128 sums per lane; 0: not built
int pw_slices(int Cx, int Cg) {
  if (Cx == 8 && Cg == 8) return 1;
  if (Cx == 16 && Cg == 16) return 4;
  if (Cx == 16 && Cg == 8) return 2;
  if (Cx == 32 && Cg == 16) return 4;
  return 0;
}

template <int CX, int CG, int S>
void pw_launch(const float *x, const float *g, const float *w, long n, int spans, unsigned grid, double *work,
               float *dx, bool want_dw, hipStream_t s) {
  if (dx && want_dw) {
    pw_bwd_kernel<CX, CG, S, true, true><<<grid, PW_THREADS, 0, s>>>(x, g, w, n, spans, work, dx);
  } else if (dx) {
    pw_bwd_kernel<CX, CG, S, true, false><<<grid, PW_THREADS, 0, s>>>(x, g, w, n, spans, work, dx);
  } else {
    pw_bwd_kernel<CX, CG, S, false, true><<<grid, PW_THREADS, 0, s>>>(x, g, w, n, spans, work, dx);
  }
}

bool overlap(const float *a, long na, const float *b, long nb) { return a < b + nb && b < a + na; }

}  // namespace

extern "C" int sa_trilinear_up_adjoint(const float *g, int B, int C, int D, int H, int W, int Dp, int Hp, int Wp,
                                       float *dp, void *stream) {
  SA_REQUIRE(g && dp, "sa_trilinear_up_adjoint: null pointer (g / dp)");
  SA_REQUIRE(B > 0 && C > 0 && D > 1 && H > 1 && W > 1 && Dp > 0 && Hp > 0 && Wp > 0,
             "sa_trilinear_up_adjoint: bad shape B %d C %d, %d x %d x %d <- %d x %d x %d (D, H, W at least 2)", B, C, D,
             H, W, Dp, Hp, Wp);
  SA_REQUIRE(2L * (Dp - 1) <= D - 1 && 2L * (Hp - 1) <= H - 1 && 2L * (Wp - 1) <= W - 1,
             "sa_trilinear_up_adjoint: bad shape (the low-resolution branch must be at most half size: 2 (n - 1) <= "
             "N - 1 per axis)");
  const long n = (long)D * H * W, np = (long)Dp * Hp * Wp;
  SA_REQUIRE(n < (1L << 31), "sa_trilinear_up_adjoint: bad shape (D*H*W = %ld must be below 2^31)", n);
  const int tilesD = (Dp + UP_DZ - 1) / UP_DZ, tilesH = (Hp + UP_HY - 1) / UP_HY;
  const long blocks = (long)B * C * tilesD * tilesH;
  SA_REQUIRE(blocks <= 0x7fffffffL, "sa_trilinear_up_adjoint: bad shape (%ld blocks exceed 2^31 - 1)", blocks);
  SA_REQUIRE(!overlap(dp, (long)B * C * np, g, (long)B * C * n), "sa_trilinear_up_adjoint: dp overlaps g");
  // area_pixel_compute_scale(align_corners=True) = (in - 1) / (out - 1), as sa_conv3d_pointwise_upcat forms it
  const float sd = (float)(Dp - 1) / (float)(D - 1), sh = (float)(Hp - 1) / (float)(H - 1),
              sw = (float)(Wp - 1) / (float)(W - 1);
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  up_adjoint_kernel<<<(unsigned)blocks, 64, 0, s>>>(g, D, H, W, Dp, Hp, Wp, sd, sh, sw, tilesD, tilesH, dp);
  return sa::check_launch("sa_trilinear_up_adjoint");
}

extern "C" long sa_conv3d_pointwise_backward_work(int Cx, int Cg, int B, long n) {
  const int S = pw_slices(Cx, Cg);
  if (S == 0 || B <= 0 || n <= 0) return -1;
  return (long)B * ((n + PW_SPAN - 1) / PW_SPAN) * PW_WAVES * (Cx / S * Cg);
}

extern "C" int sa_conv3d_pointwise_backward(const float *x, const float *g, const float *w, int Cx, int Cg, int B,
                                            long n, double *work, float *dx, float *dw, void *stream) {
  SA_REQUIRE(x && g && w, "sa_conv3d_pointwise_backward: null pointer (x / g / w)");
  SA_REQUIRE(B > 0 && n > 0, "sa_conv3d_pointwise_backward: bad shape B %d n %ld", B, n);
  SA_REQUIRE(n < (1L << 31), "sa_conv3d_pointwise_backward: bad shape (n = %ld cells must be below 2^31)", n);
  SA_REQUIRE(dx || dw, "sa_conv3d_pointwise_backward: no output (dx and dw are both null)");
  SA_REQUIRE(!dw || work, "sa_conv3d_pointwise_backward: null pointer (dw needs work)");
  const int S = pw_slices(Cx, Cg);
  if (S == 0) {
    sa::set_error("sa_conv3d_pointwise_backward: no kernel built for %d x %d (built: 8 x 8, 16 x 16, 16 x 8, 32 x 16)",
                  Cx, Cg);
    return SA_E_ARG;
  }
  const long spans = (n + PW_SPAN - 1) / PW_SPAN, blocks = (long)B * spans;
  SA_REQUIRE(blocks <= 0x7fffffffL, "sa_conv3d_pointwise_backward: bad shape (%ld blocks exceed 2^31 - 1)", blocks);
  if (dx)
    SA_REQUIRE(!overlap(dx, (long)B * Cx * n, x, (long)B * Cx * n) && !overlap(dx, (long)B * Cx * n, g, (long)B * Cg * n) &&
                   !overlap(dx, (long)B * Cx * n, w, (long)Cx * Cg),
               "sa_conv3d_pointwise_backward: dx overlaps x, g or w");
  if (dw)
    SA_REQUIRE(!overlap(dw, (long)Cx * Cg, x, (long)B * Cx * n) && !overlap(dw, (long)Cx * Cg, g, (long)B * Cg * n) &&
                   !overlap(dw, (long)Cx * Cg, w, (long)Cx * Cg),
               "sa_conv3d_pointwise_backward: dw overlaps x, g or w");
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  const unsigned grid = (unsigned)blocks;
  if (Cx == 8 && Cg == 8) pw_launch<8, 8, 1>(x, g, w, n, (int)spans, grid, work, dx, dw != nullptr, s);
  if (Cx == 16 && Cg == 16) pw_launch<16, 16, 4>(x, g, w, n, (int)spans, grid, work, dx, dw != nullptr, s);
  if (Cx == 16 && Cg == 8) pw_launch<16, 8, 2>(x, g, w, n, (int)spans, grid, work, dx, dw != nullptr, s);
  if (Cx == 32 && Cg == 16) pw_launch<32, 16, 4>(x, g, w, n, (int)spans, grid, work, dx, dw != nullptr, s);
  if (dw) pw_fold_kernel<<<(unsigned)(Cx * Cg), 64, 0, s>>>(work, blocks, S, Cx / S, Cg, dw);
  return sa::check_launch("sa_conv3d_pointwise_backward");
}

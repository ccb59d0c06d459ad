// Backward of the correlation plug-in (HipCorrBlock1D under autograd): the adjoints of the lookup
// (corr_lookup.hip, lookup_kernel), of the avg-pool pyramid (corr_volume.hip,
// pyramid_from_volume_kernel) and of the correlation volume (CorrBlock1D.corr, corr.py:117-132).
//
// All three are fp32 and deterministic: no floating-point atomics, one fixed summation order per
// output element, no split of a contraction across waves or blocks.
#include "sa_common.h"

namespace {

// ------------------------------------------------------------------------------------ lookup
// A block owns `np` consecutive pixels and builds the cells [c0, c0 + chw) of their pyramid rows
// in LDS: zero, then one lane per (pixel, level) walks that level's taps in ascending order and
// adds g e into cell xi and g w into cell xi + 1 (a pixel's row is private to it and a level's
// cells to one lane, so the order of every cell's sum is the tap order), then the block copies the
// rows out.  With chw == row_stride (every row that fits the LDS budget) the block's rows are one
// contiguous span of global memory, written as float4.  xi, w and e are the forward's own
// expression sequence (corr_lookup.hip:42-53), evaluated per tap: near integer coordinates the
// floors of neighbouring taps repeat or skip a cell, so cells are never indexed relative to a base.
constexpr int LB_LDS = 12288;   // floats (48 KiB: three blocks per CU)
constexpr int LB_MAXP = 64;     // pixels per block (x 4 levels = 256 lanes)

struct BGeo {
  int H, W1, L, r, np, chw;
  long rs, cbs, gbs;
  int off[4], wid[4];
};

template <bool VEC>
__global__ __launch_bounds__(256) void lookup_backward_kernel(const float *__restrict__ go,
                                                              const float *__restrict__ cx, BGeo g, long npix,
                                                              float *__restrict__ gp) {
  __shared__ __attribute__((aligned(16))) float rows[LB_LDS];
  const long p0 = (long)blockIdx.x * g.np;
  const int c0 = (int)blockIdx.y * g.chw;
  const int npb = (int)min((long)g.np, npix - p0);
  const int cw = min(g.chw, (int)(g.rs - c0));
  const int n = npb * cw;   // <= np * chw <= LB_LDS
  const int tid = threadIdx.x;
  for (int i = 4 * tid; i < n; i += 1024) *reinterpret_cast<float4 *>(rows + i) = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  if (tid < npb * g.L) {
    const int l = tid / npb, pp = tid - l * npb;   // consecutive lanes: consecutive pixels
    const long p = p0 + pp;
    const long hw = (long)g.H * g.W1;
    const long b = p / hw, rem = p % hw;
    const float x = cx[b * g.cbs + rem];
    const int K = 2 * g.r + 1;
    const float *__restrict__ gl = go + b * g.gbs + (long)l * K * hw + rem;
    float *__restrict__ row = rows + pp * cw;
    const int Wl = g.wid[l];
    const int base = g.off[l] - c0;   // LDS index of the level's cell 0
    const float xl = x / (float)(1 << l);
    const float denom = (float)(Wl - 1);
    const float sf = (float)(Wl - 1) / 2.0f;
    for (int t = -g.r; t <= g.r; ++t) {
      const float x0 = (float)t + xl;
      const float xg = 2.0f * x0 / denom - 1.0f;
      const float ix = (xg + 1.0f) * sf;
      float xw = floorf(ix);
      const float w = ix - xw;
      const float e = 1.0f - w;
      xw = fminf(fmaxf(xw, -2.0f), (float)Wl + 1.0f);   // keep the int conversion defined
      const int xi = (int)xw;
      const float gv = gl[(long)(t + g.r) * hw];
      const int i0 = base + xi, i1 = i0 + 1;
      if (xi >= 0 && xi <= Wl - 1 && i0 >= 0 && i0 < cw) row[i0] += gv * e;
      if (xi + 1 >= 0 && xi + 1 <= Wl - 1 && i1 >= 0 && i1 < cw) row[i1] += gv * w;
    }
  }
  __syncthreads();
  if (VEC) {   // rs, chw (so cw and n) multiples of 4, gp 16-byte aligned
    for (int i = 4 * tid; i < n; i += 1024) {
      const int pp = i / cw, cc = i - pp * cw;
      *reinterpret_cast<float4 *>(gp + (p0 + pp) * g.rs + c0 + cc) = *reinterpret_cast<const float4 *>(rows + i);
    }
  } else {
    for (int i = tid; i < n; i += 256) {
      const int pp = i / cw, cc = i - pp * cw;
      gp[(p0 + pp) * g.rs + c0 + cc] = rows[i];
    }
  }
}

// ----------------------------------------------------------------------------------- pyramid
// One thread per 4 consecutive level-0 cells k of a row: grad_volume[k] = sum over l ascending of
// 2^-l grad_level_l[k >> l] (the scale is exact), levels whose width floors away cell k >> l
// skipped.  Consecutive threads are consecutive cells: every read and the store are coalesced.
struct PGeo {
  int L, W2, nq;
  long rs, ors;
  int off[4], wid[4];
};

template <bool VEC>
__global__ __launch_bounds__(256) void pyramid_backward_kernel(const float *__restrict__ gp, long total, PGeo g,
                                                               float *__restrict__ gv) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long row = idx / g.nq;
  const int k0 = 4 * (int)(idx - row * g.nq);
  const float *__restrict__ src = gp + row * g.rs;
  float *__restrict__ dst = gv + row * g.ors;
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = k0 + i;
    float s = 0.f;
    if (k < g.W2) {
      s = src[k];
      float scale = 0.5f;
      for (int l = 1; l < g.L; ++l, scale *= 0.5f) {
        const int kl = k >> l;
        if (kl < g.wid[l]) s += scale * src[g.off[l] + kl];
      }
    }
    v[i] = s;
  }
  if (VEC && k0 + 3 < g.W2) {
    *reinterpret_cast<float4 *>(dst + k0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (k0 + i < g.W2) dst[k0 + i] = v[i];
  }
}

// ------------------------------------------------------------------------------------ volume
// Per image row (b, h) the two adjoints of V = f2^T f3 / sqrt(C) are GEMMs with M = C:
//   grad_fmap2 [C x W1] = f3 [C x W2] . G^T [W2 x W1]      (BK: both operands contiguous along K)
//   grad_fmap3 [C x W2] = f2 [C x W1] . G   [W1 x W2]      (!BK: G contiguous along N)
// on v_mfma_f32_32x32x2_f32 (A lane l: A[l & 31][l >> 5], B lane l: B[l >> 5][l & 31]; exact fp32
// products, fp32 accumulation, K ascending in one chain per element: nothing is split).  A block
// computes 128 (channels) x 64 (pixels) with 4 waves of 32 x 64 (two 32x32 accumulators), K in
// slices of 32 through LDS with the next slice's loads in flight under the MFMAs.  Operands
// contiguous along K sit in LDS as [row][33] (odd pitch: the lanes' rows fall in distinct banks).
// Ragged tiles are zero-filled on load and masked on store, so any C, W1, W2 >= 1 runs.
constexpr int VB_M = 128, VB_N = 64, VB_K = 32, VB_P = VB_K + 1;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct VGeo {
  int C, H, W1, N, K, tilesM, tilesN;
  long vrs;
};

template <bool BK>
__global__ __launch_bounds__(256) void volume_backward_kernel(const float *__restrict__ G,
                                                              const float *__restrict__ fa, VGeo g, float sqrt_c,
                                                              float *__restrict__ out) {
  __shared__ float As[VB_M * VB_P];
  __shared__ float Bs[VB_N * VB_P];   // BK: [n][33]; else [k][64]
  const unsigned wid = sa::xcd_remap(blockIdx.x, gridDim.x);
  const int mt = wid % g.tilesM, rest = wid / g.tilesM;
  const int nt = rest % g.tilesN, bh = rest / g.tilesN;
  const int b = bh / g.H, h = bh % g.H;
  const int m0 = mt * VB_M, n0 = nt * VB_N;
  const long astride = (long)g.H * g.K;                            // channel stride of the A feature map
  const float *__restrict__ ap = fa + (long)b * g.C * astride + (long)h * g.K;
  const float *__restrict__ gb = G + (long)bh * g.W1 * g.vrs;     // the image row's [W1][W2] slice
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;

  float ra[16], rb[8];
  auto load = [&](int kc) {
    const int kk = t & 31, r0 = t >> 5;
    const bool kok = kc + kk < g.K;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int m = m0 + r0 + 8 * i;
      ra[i] = (kok && m < g.C) ? ap[(long)m * astride + kc + kk] : 0.f;
    }
    if (BK) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int nn = n0 + r0 + 8 * i;
        rb[i] = (kok && nn < g.N) ? gb[(long)nn * g.vrs + kc + kk] : 0.f;
      }
    } else {
      const int nn = n0 + (t & 63), k0 = kc + (t >> 6);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = k0 + 4 * i;
        rb[i] = (k < g.K && nn < g.N) ? gb[(long)k * g.vrs + nn] : 0.f;
      }
    }
  };
  auto store = [&]() {
    const int kk = t & 31, r0 = t >> 5;
#pragma unroll
    for (int i = 0; i < 16; ++i) As[(r0 + 8 * i) * VB_P + kk] = ra[i];
    if (BK) {
#pragma unroll
      for (int i = 0; i < 8; ++i) Bs[(r0 + 8 * i) * VB_P + kk] = rb[i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) Bs[((t >> 6) + 4 * i) * VB_N + (t & 63)] = rb[i];
    }
  };

  f32x16 acc0 = {0.f}, acc1 = {0.f};
  const int col = lane & 31, hi = lane >> 5;
  load(0);
  for (int kc = 0; kc < g.K; kc += VB_K) {
    __syncthreads();   // the previous slice is consumed
    store();
    __syncthreads();
    if (kc + VB_K < g.K) load(kc + VB_K);
#pragma unroll
    for (int kk = 0; kk < VB_K; kk += 2) {
      const float a = As[(w * 32 + col) * VB_P + kk + hi];
      const float b0 = BK ? Bs[col * VB_P + kk + hi] : Bs[(kk + hi) * VB_N + col];
      const float b1 = BK ? Bs[(32 + col) * VB_P + kk + hi] : Bs[(kk + hi) * VB_N + 32 + col];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
    }
  }

  float *__restrict__ op = out + ((long)b * g.C * g.H + h) * g.N;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int c = m0 + w * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
    if (c >= g.C) continue;
    float *__restrict__ o = op + (long)c * g.H * g.N;
    const int na = n0 + col, nb = n0 + 32 + col;
    if (na < g.N) o[na] = acc0[r] / sqrt_c;
    if (nb < g.N) o[nb] = acc1[r] / sqrt_c;
  }
}

}  // namespace

extern "C" int sa_corr_lookup_backward(const float *grad_out, long grad_bstride, const float *coords_x,
                                       long coords_bstride, int B, int H, int W1, int W2, int num_levels, int radius,
                                       float *grad_pyramid, long row_stride, void *stream) {
  SA_REQUIRE(grad_out && coords_x && grad_pyramid, "sa_corr_lookup_backward: null pointer");
  SA_REQUIRE(B > 0 && H > 0 && W1 > 0 && W2 > 0, "sa_corr_lookup_backward: empty shape");
  SA_REQUIRE(num_levels >= 1 && num_levels <= 4, "sa_corr_lookup_backward: num_levels must be 1..4");
  SA_REQUIRE(radius >= 0 && radius <= 16, "sa_corr_lookup_backward: radius must be 0..16");
  SA_REQUIRE(sa_pyramid_level_width(W2, num_levels - 1) >= 2,
             "sa_corr_lookup_backward: level %d of width %d is too narrow to sample", num_levels - 1,
             sa_pyramid_level_width(W2, num_levels - 1));
  SA_REQUIRE(row_stride >= sa_pyramid_level_offset(W2, num_levels) && row_stride < (1L << 31),
             "sa_corr_lookup_backward: row_stride out of range");
  SA_REQUIRE(grad_bstride >= (long)num_levels * (2 * radius + 1) * H * W1,
             "sa_corr_lookup_backward: grad_out batch stride too small");
  SA_REQUIRE(coords_bstride >= (long)H * W1, "sa_corr_lookup_backward: coords batch stride too small");
  BGeo g{};
  g.H = H;
  g.W1 = W1;
  g.L = num_levels;
  g.r = radius;
  g.rs = row_stride;
  g.cbs = coords_bstride;
  g.gbs = grad_bstride;
  for (int i = 0; i < 4; ++i) {
    g.off[i] = sa_pyramid_level_offset(W2, i);
    g.wid[i] = sa_pyramid_level_width(W2, i);
  }
  // rows that fit the LDS budget whole: as many pixels per block as fit; longer rows: one pixel,
  // LB_LDS cells at a time
  if (row_stride <= LB_LDS) {
    g.chw = (int)row_stride;
    g.np = LB_LDS / g.chw < LB_MAXP ? LB_LDS / g.chw : LB_MAXP;
  } else {
    g.chw = LB_LDS;
    g.np = 1;
  }
  const long npix = (long)B * H * W1;
  const long nblk = (npix + g.np - 1) / g.np, nchunk = (row_stride + g.chw - 1) / g.chw;
  SA_REQUIRE(nblk < (1L << 31) && nchunk <= 65535, "sa_corr_lookup_backward: grid too large");
  const bool vec = row_stride % 4 == 0 && reinterpret_cast<uintptr_t>(grad_pyramid) % 16 == 0;
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  const dim3 grid((unsigned)nblk, (unsigned)nchunk);
  if (vec)
    lookup_backward_kernel<true><<<grid, 256, 0, s>>>(grad_out, coords_x, g, npix, grad_pyramid);
  else
    lookup_backward_kernel<false><<<grid, 256, 0, s>>>(grad_out, coords_x, g, npix, grad_pyramid);
  return sa::check_launch("sa_corr_lookup_backward");
}

extern "C" int sa_corr_pyramid_backward(const float *grad_pyramid, long rows, int W2, long row_stride, int num_levels,
                                        float *grad_volume, long out_row_stride, void *stream) {
  SA_REQUIRE(grad_pyramid && grad_volume, "sa_corr_pyramid_backward: null pointer");
  SA_REQUIRE(rows > 0 && W2 > 0 && out_row_stride >= W2, "sa_corr_pyramid_backward: bad shape");
  SA_REQUIRE(num_levels >= 1 && num_levels <= 4, "sa_corr_pyramid_backward: num_levels must be 1..4");
  SA_REQUIRE(row_stride >= sa_pyramid_level_offset(W2, num_levels), "sa_corr_pyramid_backward: row_stride too small");
  PGeo g{};
  g.L = num_levels;
  g.W2 = W2;
  g.nq = (W2 + 3) / 4;
  g.rs = row_stride;
  g.ors = out_row_stride;
  for (int i = 0; i < 4; ++i) {
    g.off[i] = sa_pyramid_level_offset(W2, i);
    g.wid[i] = sa_pyramid_level_width(W2, i);
  }
  const long total = rows * g.nq, nblk = (total + 255) / 256;
  SA_REQUIRE(nblk < (1L << 31), "sa_corr_pyramid_backward: grid too large");
  const bool vec = out_row_stride % 4 == 0 && reinterpret_cast<uintptr_t>(grad_volume) % 16 == 0;
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  if (vec)
    pyramid_backward_kernel<true><<<(unsigned)nblk, 256, 0, s>>>(grad_pyramid, total, g, grad_volume);
  else
    pyramid_backward_kernel<false><<<(unsigned)nblk, 256, 0, s>>>(grad_pyramid, total, g, grad_volume);
  return sa::check_launch("sa_corr_pyramid_backward");
}

extern "C" int sa_corr_volume_backward(const float *grad_volume, long vol_row_stride, const float *fmap2,
                                       const float *fmap3, int B, int C, int H, int W1, int W2, float sqrt_c,
                                       float *grad_fmap2, float *grad_fmap3, void *stream) {
  SA_REQUIRE(grad_volume && fmap2 && fmap3 && (grad_fmap2 || grad_fmap3), "sa_corr_volume_backward: null pointer");
  SA_REQUIRE(B > 0 && C > 0 && H > 0 && W1 > 0 && W2 > 0, "sa_corr_volume_backward: empty shape");
  SA_REQUIRE(vol_row_stride >= W2, "sa_corr_volume_backward: volume row stride too small");
  SA_REQUIRE(sqrt_c > 0.0f, "sa_corr_volume_backward: sqrt_c must be positive");
  const int tilesM = (C + VB_M - 1) / VB_M;
  const long nb2 = (long)B * H * tilesM * ((W1 + VB_N - 1) / VB_N);
  const long nb3 = (long)B * H * tilesM * ((W2 + VB_N - 1) / VB_N);
  SA_REQUIRE(nb2 < (1L << 31) && nb3 < (1L << 31), "sa_corr_volume_backward: grid too large");
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  VGeo g{};
  g.C = C;
  g.H = H;
  g.W1 = W1;
  g.tilesM = tilesM;
  g.vrs = vol_row_stride;
  if (grad_fmap2) {   // N = W1 (j), K = W2 (k): A = fmap3
    g.N = W1;
    g.K = W2;
    g.tilesN = (W1 + VB_N - 1) / VB_N;
    volume_backward_kernel<true><<<(unsigned)nb2, 256, 0, s>>>(grad_volume, fmap3, g, sqrt_c, grad_fmap2);
    const int rc = sa::check_launch("sa_corr_volume_backward");
    if (rc != SA_OK) return rc;
  }
  if (grad_fmap3) {   // N = W2 (k), K = W1 (j): A = fmap2
    g.N = W2;
    g.K = W1;
    g.tilesN = (W2 + VB_N - 1) / VB_N;
    volume_backward_kernel<false><<<(unsigned)nb3, 256, 0, s>>>(grad_volume, fmap2, g, sqrt_c, grad_fmap3);
    return sa::check_launch("sa_corr_volume_backward");
  }
  return SA_OK;
}

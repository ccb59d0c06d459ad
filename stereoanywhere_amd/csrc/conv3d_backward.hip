// Backward of the hourglass's stride-1 3x3x3 convs with Cin = Cout = C in {8, 16, 32} (conv3d_mfma.hip
// is their forward; hourglass.py:13-91).  With g = dL/dout [B,C,D,H,W]:
//   dx = conv3d(g, flip(w) with the channel roles swapped)     sa_conv3d_mf_scaled on a second table
//   dw[ci][tap][co] = sum_b sum_p x[b,ci,p+tap-1] g[b,co,p]    sa_conv3d_k3_backward_weight (this file)
// and the per-sample power-of-two scale that brings a gradient volume into the split-f16 range
// (sa_sample_scale, this file).
//
//   sample_scale_kernel  blocks of one sample fold max |t| as unsigned bits (the order of a maximum does
//                        not matter), the sample's last block turns it into s = 2^k.
//   bw_kernel            a block of 6 waves owns a 4 x TW tile of (h, w) of one sample over DR planes and
//                        walks along D.  Per plane it stages g's plane and x's next plane (a ring of three)
//                        into LDS as split f16 hi / lo, eight consecutive w per 16-byte entry, scaled by the
//                        samples' s.  GEMM: M = 16 ci, N = 16 co, K = 32 cells = one row's 32 consecutive w
//                        (4 K groups x 8 w), one accumulator per tap: a wave owns one kd (9 taps, 36 fp32)
//                        and, for C <= 16, every other row of the tile (C = 32: one 16-row half of ci; a
//                        block one 16-column half of co).  B (g) is one aligned ds_read_b128 per operand
//                        half and serves the 27 taps; A (x) is three aligned reads per kh (the entry before,
//                        at and after the K group's), the kw = 0 / 2 operands are built from them with
//                        v_alignbit on the packed halves.  C = 8 fills rows and columns 8..15 with copies
//                        of 0..7 and drops them.  Every kR = 1024 products the fp32 accumulators are added
//                        into float64 registers; at the end a block multiplies by the exact inverse
//                        scales, adds its row-halves' totals through LDS and writes 27 C C / NCH doubles.
//   bw_fold_kernel       one wave per dw element adds the blocks' partials in index order.
//
// Determinism: no atomics in the sums; every order is fixed by indices.
#include "split_f16.h"

namespace {

using sa::f32x4, sa::f16x8;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------- per-sample scale
constexpr int SC_THREADS = 256;
constexpr int SC_MAX_BLOCKS = 256;    // per sample
constexpr int SC_KMAX = 100;          // |k| <= 100: s, 1 / s and 2^-12 / s stay normal fp32

// s = 2^k with max |t| * s in [2^13, 2^14); 1 for an all-zero or non-finite sample
__device__ __forceinline__ int scale_exponent(unsigned amax_bits) {
  if (amax_bits == 0u || amax_bits >= 0x7f800000u) return 0;
  int e;
  frexpf(__uint_as_float(amax_bits), &e);   // max in [2^(e-1), 2^e)
  const int k = 14 - e;
  return k > SC_KMAX ? SC_KMAX : (k < -SC_KMAX ? -SC_KMAX : k);
}

__global__ __launch_bounds__(SC_THREADS) void sample_scale_kernel(const float *__restrict__ t, long n, int B, int rep,
                                                                  unsigned *__restrict__ state,
                                                                  float *__restrict__ scale, float *__restrict__ inv) {
  __shared__ unsigned red[SC_THREADS / 64];
  const int b = blockIdx.y;
  const float *p = t + (long)b * n;
  unsigned m = 0u;
  for (long i = (long)blockIdx.x * SC_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * SC_THREADS) {
    const unsigned v = __float_as_uint(p[i]) & 0x7fffffffu;   // |t|: ordered as unsigned, NaN above inf
    m = v > m ? v : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned v = (unsigned)__shfl_xor((int)m, o);
    m = v > m ? v : m;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < SC_THREADS / 64; ++k) m = red[k] > m ? red[k] : m;
    atomicMax(&state[b], m);
    __threadfence();
    const unsigned ticket = atomicAdd(&state[B + b], 1u);
    if (ticket == gridDim.x - 1) {   // the sample's last block
      __threadfence();
      const int k = scale_exponent(atomicMax(&state[b], 0u));
      const float s = ldexpf(1.0f, k);
      for (int i = 0; i < rep; ++i) scale[b * rep + i] = s;
      inv[b] = ldexpf(1.0f, -k);
    }
  }
}

// ------------------------------------------------------------------------------- weight gradient
constexpr int kR = 1024;   // products an fp32 accumulator takes before it is added into float64

template <int C>
struct BwCfg {
  static constexpr int TH = 4;                       // rows per tile
  static constexpr int TW = C == 32 ? 32 : 64;       // columns per tile
  static constexpr int KSP = C == 32 ? 1 : 2;        // waves that share a kd by rows
  static constexpr int MI = C == 32 ? 2 : 1;         // 16-row halves of ci, one wave each
  static constexpr int NCH = C == 32 ? 2 : 1;        // 16-column halves of co, one block each
  static constexpr int NCO = C / NCH;
  static constexpr int NWAVE = 3 * KSP * MI;
  static constexpr int NTHR = 64 * NWAVE;
  static constexpr int ROWS = TH + 2;
  static constexpr int CBX = TW / 8 + 2;             // 16-byte entries per staged x row: w0 - 8 .. w0 + TW + 7
  static constexpr int XCH = (ROWS * CBX) | 1;       // entries per channel, odd: 16 channels on 16 slots of a bank row
  static constexpr int CBG = TW / 8;
  static constexpr int GCH = (TH * CBG) | 1;
  static constexpr int XSLOT = 2 * C * XCH;          // one plane: [hl][ci][row][cb]
  static constexpr int XENT = 3 * XSLOT;
  static constexpr int GENT = 2 * NCO * GCH;         // [hl][co][row][cb]
  static constexpr int ENTRIES = XENT + GENT;
  static constexpr int KSTEPS = TH / KSP * (TW / 32);   // K-steps per plane per wave
  static constexpr int FLUSH = kR / 32 / KSTEPS;        // planes between two float64 additions
  static constexpr int BLOCK_OUT = 27 * C * NCO;        // doubles a block writes
  static_assert(NWAVE == 6, "six waves");
  static_assert(FLUSH >= 1 && FLUSH * KSTEPS * 32 <= kR && kR <= 1024, "fp32 chain");
  static_assert(ENTRIES * 16 <= 160 * 1024, "LDS");
  static_assert(KSP == 1 || 3 * 36 * 64 * 8 <= ENTRIES * 16, "the row-halves' totals reuse the staging LDS");
};

// x at w - 1: element j <- cur j - 1, element 0 <- prev 7 (two f16 per dword, the lower index in the low half)
__device__ __forceinline__ f16x8 shift_from_prev(f16x8 prev, f16x8 cur) {
  const u32x4 p = __builtin_bit_cast(u32x4, prev), c = __builtin_bit_cast(u32x4, cur);
  u32x4 r;
  r[0] = __builtin_amdgcn_alignbit(c[0], p[3], 16);
  r[1] = __builtin_amdgcn_alignbit(c[1], c[0], 16);
  r[2] = __builtin_amdgcn_alignbit(c[2], c[1], 16);
  r[3] = __builtin_amdgcn_alignbit(c[3], c[2], 16);
  return __builtin_bit_cast(f16x8, r);
}

// x at w + 1: element j <- cur j + 1, element 7 <- next 0
__device__ __forceinline__ f16x8 shift_from_next(f16x8 cur, f16x8 next) {
  const u32x4 c = __builtin_bit_cast(u32x4, cur), n = __builtin_bit_cast(u32x4, next);
  u32x4 r;
  r[0] = __builtin_amdgcn_alignbit(c[1], c[0], 16);
  r[1] = __builtin_amdgcn_alignbit(c[2], c[1], 16);
  r[2] = __builtin_amdgcn_alignbit(c[3], c[2], 16);
  r[3] = __builtin_amdgcn_alignbit(n[0], c[3], 16);
  return __builtin_bit_cast(f16x8, r);
}

template <int C>
__global__ __launch_bounds__((BwCfg<C>::NTHR)) void bw_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                             const float *__restrict__ sx, const float *__restrict__ sg,
                                                             int D, int H, int W, int tilesW, int tilesH, int tilesD,
                                                             int DR, double *__restrict__ work) {
  using K = BwCfg<C>;
  __shared__ f16x8 lds[K::ENTRIES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ch = blockIdx.x % K::NCH;
  const long t = blockIdx.x / K::NCH;   // (b, dz, by, bx): the block's place in work
  const int bx = (int)(t % tilesW), by = (int)(t / tilesW % tilesH), dz = (int)(t / ((long)tilesW * tilesH) % tilesD);
  const int b = (int)(t / ((long)tilesW * tilesH * tilesD));
  const int w0 = bx * K::TW, h0 = by * K::TH, d0 = dz * DR, d1 = min(d0 + DR, D);
  const long HW = (long)H * W, n = (long)D * HW;
  const float scx = sx ? sx[b] : 1.0f, scg = sg ? sg[b] : 1.0f;
  const float *xb = x + (long)b * C * n;
  const float *gb = g + ((long)b * C + ch * K::NCO) * n;

  // plane p of x (zeros outside the volume: the conv's padding) -> its ring slot
  auto stage_x = [&](int p) {
    f16x8 *dst = lds + ((p + 3) % 3) * K::XSLOT;
    const bool pin = p >= 0 && p < D;
    for (int j = tid; j < C * K::ROWS * K::CBX; j += K::NTHR) {
      const int cb = j % K::CBX, r = j / K::CBX % K::ROWS, ci = j / (K::CBX * K::ROWS);
      const int h = h0 - 1 + r, wa = w0 - 8 + 8 * cb;
      f16x8 hi{}, lo{};
      if (pin && h >= 0 && h < H && wa + 7 >= 0 && wa < W) {
        const float *src = xb + ((long)ci * D + p) * HW + (long)h * W;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int w = wa + e;
          const float v = w >= 0 && w < W ? src[w] * scx : 0.0f;
          _Float16 a, c;
          sa::split_f16(v, a, c);
          hi[e] = a;
          lo[e] = c;
        }
      }
      dst[ci * K::XCH + r * K::CBX + cb] = hi;
      dst[(C + ci) * K::XCH + r * K::CBX + cb] = lo;
    }
  };
  // plane d of g (zeros outside H x W: those cells are no outputs)
  auto stage_g = [&](int d) {
    f16x8 *dst = lds + K::XENT;
    for (int j = tid; j < K::NCO * K::TH * K::CBG; j += K::NTHR) {
      const int cb = j % K::CBG, r = j / K::CBG % K::TH, co = j / (K::CBG * K::TH);
      const int h = h0 + r, wa = w0 + 8 * cb;
      f16x8 hi{}, lo{};
      if (h < H && wa < W) {
        const float *src = gb + ((long)co * D + d) * HW + (long)h * W;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int w = wa + e;
          const float v = w < W ? src[w] * scg : 0.0f;
          _Float16 a, c;
          sa::split_f16(v, a, c);
          hi[e] = a;
          lo[e] = c;
        }
      }
      dst[co * K::GCH + r * K::CBG + cb] = hi;
      dst[(K::NCO + co) * K::GCH + r * K::CBG + cb] = lo;
    }
  };

  // the wave's kd and its share (rows for C <= 16, a half of ci for C = 32); the lane's A row and B column
  const int kd = wv % 3, sec = wv / 3;
  const int m = lane & 15, kg = lane >> 4;
  const int row0 = K::MI == 2 ? 16 * sec : 0;
  const int ci_l = row0 + (C == 8 ? (m & 7) : m);
  const int co_l = C == 8 ? (m & 7) : m;
  const int ks = K::KSP == 2 ? sec : 0;

  f32x4 acc[9];
  double tot[9][4];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    acc[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 4; ++j) tot[k][j] = 0.0;
  }
  auto flush = [&]() {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) tot[k][j] += (double)acc[k][j];
      acc[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
  };

  stage_x(d0 - 1);
  stage_x(d0);
  int chain = 0;
#pragma unroll 1
  for (int d = d0; d < d1; ++d) {
    stage_x(d + 1);   // its slot held plane d - 2, last read before the barrier that ended step d - 1
    stage_g(d);
    __syncthreads();
    const f16x8 *xs = lds + ((d + kd - 1 + 3) % 3) * K::XSLOT + ci_l * K::XCH;
    const f16x8 *gs = lds + K::XENT + co_l * K::GCH;
#pragma unroll
    for (int r = ks; r < K::TH; r += K::KSP) {
#pragma unroll
      for (int q = 0; q < K::TW / 32; ++q) {
        const f16x8 bh = gs[r * K::CBG + 4 * q + kg], bl = gs[K::NCO * K::GCH + r * K::CBG + 4 * q + kg];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          const f16x8 *a = xs + (r + kh) * K::CBX + 4 * q + kg;   // the entry before the K group's
          const f16x8 ph = a[0], chh = a[1], nh = a[2];
          const f16x8 pl = a[C * K::XCH], cl = a[C * K::XCH + 1], nl = a[C * K::XCH + 2];
          sa::mfma_split3(acc[3 * kh + 0], shift_from_prev(ph, chh), shift_from_prev(pl, cl), bh, bl);
          sa::mfma_split3(acc[3 * kh + 1], chh, cl, bh, bl);
          sa::mfma_split3(acc[3 * kh + 2], shift_from_next(chh, nh), shift_from_next(cl, nl), bh, bl);
        }
      }
    }
    if (++chain == K::FLUSH) {
      flush();
      chain = 0;
    }
    __syncthreads();
  }
  flush();

  // the sample's exact inverse scales (powers of two), then the row-halves' totals in a fixed order
  const double inv = 1.0 / ((double)scx * (double)scg);
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) tot[k][j] *= inv;
  if (K::KSP == 2) {
    double *red = reinterpret_cast<double *>(lds);   // (the loop's last barrier has passed)
    if (sec == 1) {
#pragma unroll
      for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) red[((kd * 9 + k) * 4 + j) * 64 + lane] = tot[k][j];
    }
    __syncthreads();
    if (sec == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) tot[k][j] += red[((kd * 9 + k) * 4 + j) * 64 + lane];
    }
  }
  // the lane holds rows ci = row0 + 4 kg + j and column co = lane & 15 of its nine taps
  if ((K::KSP == 1 || sec == 0) && (C != 8 || (kg < 2 && m < 8))) {
    double *o = work + t * (27L * C * C) + ch * K::NCO + m;
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) o[((long)(row0 + 4 * kg + j) * 27 + kd * 9 + k) * C] = tot[k][j];
  }
}

// one wave per dw element: the nblk block partials in index order, lanes strided, then the DPP tree
__global__ __launch_bounds__(64) void bw_fold_kernel(const double *__restrict__ work, long nblk, int E,
                                                     float *__restrict__ dw) {
  double s = 0.0;
  for (long q = threadIdx.x; q < nblk; q += 64) s += work[q * E + blockIdx.x];
  s = sa::wave_sum_dpp_lane63(s);
  if (threadIdx.x == 63) dw[blockIdx.x] = (float)s;
}

struct BwGeo {
  int tilesW, tilesH, tilesD, DR;
  long tiles;   // B tilesD tilesH tilesW
};

inline bool bw_shape(int C) { return C == 8 || C == 16 || C == 32; }

BwGeo bw_geo(int C, int B, int D, int H, int W) {
  const int tw = C == 32 ? 32 : 64, nch = C == 32 ? 2 : 1;
  BwGeo g{(W + tw - 1) / tw, (H + 3) / 4, 1, 0, 0};
  const int planes = sa_conv3d_mf_get_planes();   // the forward's test / A-B override cuts D here too
  int dr = planes > 0 ? planes : D;
  if (planes <= 0) {
    // halve the planes per block until the grid holds two blocks per CU or a block is down to 8 planes
    const long per = (long)B * g.tilesW * g.tilesH * nch;
    while (dr > 8 && per * ((D + dr - 1) / dr) < 2 * 256) dr = (dr + 1) / 2;
  }
  g.DR = dr;
  g.tilesD = (D + dr - 1) / dr;
  g.tiles = (long)B * g.tilesD * g.tilesH * g.tilesW;
  return g;
}

bool overlap(const void *a, long na, const void *b, long nb) {
  const char *p = static_cast<const char *>(a), *q = static_cast<const char *>(b);
  return p < q + nb && q < p + na;
}

}  // namespace

extern "C" int sa_sample_scale(const float *t, int B, long n, int rep, void *state_, float *scale, float *inv,
                               void *stream) {
  unsigned *state = static_cast<unsigned *>(state_);
  SA_REQUIRE(t && state && scale && inv, "sa_sample_scale: null pointer (t / state / scale / inv)");
  SA_REQUIRE(B > 0 && B <= 65535 && n > 0 && rep > 0, "sa_sample_scale: bad shape B %d (1 .. 65535) n %ld rep %d", B, n,
             rep);
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  if (hipMemsetAsync(state, 0, 2 * (size_t)B * sizeof(unsigned), s) != hipSuccess) return sa::check_launch("sa_sample_scale");
  const long want = (n + SC_THREADS * 16L - 1) / (SC_THREADS * 16L);
  const unsigned nb = (unsigned)(want < SC_MAX_BLOCKS ? want : SC_MAX_BLOCKS);
  sample_scale_kernel<<<dim3(nb, (unsigned)B), SC_THREADS, 0, s>>>(t, n, B, rep, state, scale, inv);
  return sa::check_launch("sa_sample_scale");
}

extern "C" long sa_conv3d_k3_backward_weight_work(int C, int B, int D, int H, int W) {
  if (!bw_shape(C) || B <= 0 || D <= 0 || H <= 0 || W <= 0) return -1;
  return bw_geo(C, B, D, H, W).tiles * 27L * C * C;
}

extern "C" int sa_conv3d_k3_backward_weight(const float *x, const float *g, int C, int B, int D, int H, int W,
                                            const float *x_scale, const float *g_scale, double *work, float *dw,
                                            void *stream) {
  SA_REQUIRE(x && g && work && dw, "sa_conv3d_k3_backward_weight: null pointer (x / g / work / dw)");
  SA_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "sa_conv3d_k3_backward_weight: bad shape B %d, %d x %d x %d", B, D, H, W);
  if (!bw_shape(C)) {
    sa::set_error("sa_conv3d_k3_backward_weight: no kernel built for %d -> %d channels (built: 8 -> 8, 16 -> 16, 32 -> 32)",
                  C, C);
    return SA_E_ARG;
  }
  const long n = (long)D * H * W;
  SA_REQUIRE(n < (1L << 30), "sa_conv3d_k3_backward_weight: bad shape (D*H*W = %ld cells must be below 2^30)", n);
  const BwGeo geo = bw_geo(C, B, D, H, W);
  const long blocks = geo.tiles * (C == 32 ? 2 : 1);
  SA_REQUIRE(blocks <= 0x7fffffffL, "sa_conv3d_k3_backward_weight: bad shape (%ld blocks exceed 2^31 - 1)", blocks);
  const long vol = (long)B * C * n * 4, dwb = 27L * C * C * 4, wkb = geo.tiles * 27L * C * C * 8;
  SA_REQUIRE(!overlap(dw, dwb, x, vol) && !overlap(dw, dwb, g, vol) && !overlap(dw, dwb, work, wkb),
             "sa_conv3d_k3_backward_weight: dw overlaps x, g or work");
  SA_REQUIRE(!overlap(work, wkb, x, vol) && !overlap(work, wkb, g, vol),
             "sa_conv3d_k3_backward_weight: work overlaps x or g");
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
#define SA_BW(CC)                                                                                                     \
  bw_kernel<CC><<<(unsigned)blocks, BwCfg<CC>::NTHR, 0, s>>>(x, g, x_scale, g_scale, D, H, W, geo.tilesW, geo.tilesH, \
                                                             geo.tilesD, geo.DR, work)
  if (C == 8) SA_BW(8);
  else if (C == 16) SA_BW(16);
  else SA_BW(32);
#undef SA_BW
  bw_fold_kernel<<<(unsigned)(27 * C * C), 64, 0, s>>>(work, geo.tiles, 27 * C * C, dw);
  return sa::check_launch("sa_conv3d_k3_backward_weight");
}

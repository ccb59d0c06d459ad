// The close of a training-time hourglass layer on a volume a torch conv produced (hourglass.py:61-91,
// submodule.py:25-53, 113-140): InstanceNorm3d + LeakyReLU (+ the DoubleFeatureAtt gate) as one
// differentiable operator.  With n = D H W cells per (b, c):
//   xh = (x - mean) rstd,  a = lrelu(xh),  G = gl[h,w] gr[h,d],  out = G a   (out = a without a gate).
// The forward's apply is sa_vol_apply (conv3d_fused.hip), its statistics' fold sa_instnorm_finalize;
// this file adds the statistics pass over an existing volume and the backward.
//
// Volumes are [B, C, D = W2, H, W = W1] fp32, contiguous; gl [B,C,H,W] and gr [B,C,H,D] are the
// sigmoid'ed maps at the volume's own resolution.  All kernels are memory-bound streams; a lane moves
// 16 bytes along W per step at dword alignment (a row of a volume with W % 4 != 0 does not start on a
// 16-byte boundary), the W % 4 tail goes as dwords.
//
//   close_stats_kernel       a block sums a contiguous run of STAT_CHUNK cells of one (b, c) in float64
//                            -> one (sum, sum^2) partial per block, for sa_instnorm_finalize.
//   close_bwd_reduce_kernel  one block per (b, c, h): lanes along W (a tile of 256 columns per round),
//                            the block's waves take d = wave, wave + WAVES, ... serially.  A lane keeps
//                            its four columns' dgl sums over d; each d-step ends in one wave reduction
//                            along W for dgr[h,d]; S1 = sum u and S2 = sum u xh are kept per lane in
//                            float64 (a row's four cells first in fp32) -> one partial per block.
//   close_bwd_fold_kernel    one wave per (b, c) folds the H partials -> (S1 / n, S2 / n).
//   close_bwd_apply_kernel   dx = rstd (u - S1/n - xh S2/n), a wave per row like volume_stage.hip.
// with u = g G (xh > 0 ? 1 : slope) (torch's leaky_relu rule: the slope at xh == 0).
//
// Determinism: no atomics; every sum's order is fixed by indices (a lane's serial d or index loop,
// the DPP tree of sa_common.h, waves 0..WAVES-1 in order, column tiles in order).
#include "sa_common.h"

namespace {

// 16 bytes at dword alignment (global loads and stores of gfx950 need no more)
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

constexpr int WAVES = 4;
constexpr int THREADS = 64 * WAVES;
constexpr long STAT_CHUNK = 16L * 4 * THREADS;   // cells per statistics block: 16 steps of 16 bytes per lane
constexpr int TILE_W = 4 * 64;                   // columns per round of the reduce kernel
constexpr int ROWS_PER_WAVE = 4;

// two float64 sums of a block (every thread calls) -> their totals in every thread; waves in order
__device__ __forceinline__ void block_sum2(double &a, double &b) {
  __shared__ double part[2][WAVES];
  a = sa::wave_sum_dpp_lane63(a);
  b = sa::wave_sum_dpp_lane63(b);
  if ((threadIdx.x & 63) == 63) {
    part[0][threadIdx.x >> 6] = a;
    part[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  a = part[0][0];
  b = part[1][0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) {
    a += part[0][w];
    b += part[1][w];
  }
}

__global__ __launch_bounds__(THREADS) void close_stats_kernel(const float *__restrict__ x, long n, int parts,
                                                              double *__restrict__ partial) {
  const long bc = blockIdx.x / parts;
  const long lo = (long)(blockIdx.x % parts) * STAT_CHUNK;
  const long len = n - lo < STAT_CHUNK ? n - lo : STAT_CHUNK;
  const float *p = x + bc * n + lo;
  const int nvec = (int)(len >> 2);
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < nvec; i += THREADS) {
    const f32x4u v = *reinterpret_cast<const f32x4u *>(p + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double t = (double)v[e];
      s += t;
      q += t * t;
    }
  }
  for (int i = 4 * nvec + threadIdx.x; i < len; i += THREADS) {
    const double t = (double)p[i];
    s += t;
    q += t * t;
  }
  block_sum2(s, q);
  if (threadIdx.x == 0) {
    partial[2L * blockIdx.x] = s;
    partial[2L * blockIdx.x + 1] = q;
  }
}

// a lane's four columns of a row; columns past the row's end read as 0
__device__ __forceinline__ void load4(const float *__restrict__ p, int valid, float (&v)[4]) {
  if (valid == 4) {
    const f32x4u t = *reinterpret_cast<const f32x4u *>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = t[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < valid ? p[e] : 0.0f;
  }
}

template <bool GATED>
__global__ __launch_bounds__(THREADS) void close_bwd_reduce_kernel(
    const float *__restrict__ x, const float *__restrict__ g, const float *__restrict__ mean,
    const float *__restrict__ rstd, const float *__restrict__ gl, const float *__restrict__ gr, float slope, int D,
    int H, int W, double *__restrict__ partial, float *__restrict__ dgl, float *__restrict__ dgr) {
  __shared__ float red[WAVES][TILE_W];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long bch = blockIdx.x;   // (b c) H + h: the row of both gate maps
  const long bc = bch / H;
  const int h = (int)(bch % H);
  const float mu = mean[bc], rs = rstd[bc];
  const long hw = (long)H * W;
  const long base = bc * D * hw + (long)h * W;
  double s1 = 0.0, s2 = 0.0;
  for (int w0 = 0; w0 < W; w0 += TILE_W) {
    const int w = w0 + 4 * lane;
    const int valid = W - w >= 4 ? 4 : (W - w > 0 ? W - w : 0);
    float glv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (GATED) load4(gl + bch * W + w, valid, glv);
    for (int d = wave; d < D; d += WAVES) {
      float xv[4], gv[4];
      load4(x + base + d * hw + w, valid, xv);
      load4(g + base + d * hw + w, valid, gv);   // 0 past the row's end: those cells add 0 to every sum
      const float grd = GATED ? gr[bch * D + d] : 1.0f;
      float p1 = 0.0f, p2 = 0.0f, pr = 0.0f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (xv[e] - mu) * rs;
        const float k = xh > 0.0f ? 1.0f : slope;
        float u = gv[e] * k;
        if (GATED) {
          const float ga = gv[e] * (xh * k);   // g a
          acc[e] += ga * grd;
          pr += ga * glv[e];
          u = gv[e] * (glv[e] * grd) * k;
        }
        p1 += u;
        p2 += u * xh;
      }
      s1 += (double)p1;
      s2 += (double)p2;
      if (GATED && dgr) {
        pr = sa::wave_sum_dpp(pr);
        if (lane == 0) {   // a later tile adds to what this same lane stored for the tile before
          const long i = bch * D + d;
          dgr[i] = w0 == 0 ? pr : dgr[i] + pr;
        }
      }
    }
    if (GATED && dgl) {
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wave][4 * lane + e] = acc[e];
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float t = red[0][4 * lane + e];
#pragma unroll
          for (int v = 1; v < WAVES; ++v) t += red[v][4 * lane + e];
          if (e < valid) dgl[bch * W + w + e] = t;
        }
      }
      __syncthreads();
    }
  }
  block_sum2(s1, s2);
  if (partial && threadIdx.x == 0) {
    partial[2 * bch] = s1;
    partial[2 * bch + 1] = s2;
  }
}

// one wave per (b, c): sums[bc] = (S1, S2) / n from the H block partials, lanes strided, then the DPP tree
__global__ __launch_bounds__(64) void close_bwd_fold_kernel(const double *__restrict__ partial, int parts, double n,
                                                            double *__restrict__ sums) {
  const long bc = blockIdx.x;
  const double *p = partial + bc * parts * 2;
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < parts; i += 64) {
    a += p[2 * i];
    b += p[2 * i + 1];
  }
  a = sa::wave_sum_dpp_lane63(a);
  b = sa::wave_sum_dpp_lane63(b);
  if (threadIdx.x == 63) {
    sums[2 * bc] = a / n;
    sums[2 * bc + 1] = b / n;
  }
}

template <bool GATED>
__global__ __launch_bounds__(THREADS) void close_bwd_apply_kernel(
    const float *__restrict__ x, const float *__restrict__ g, const float *__restrict__ mean,
    const float *__restrict__ rstd, const float *__restrict__ gl, const float *__restrict__ gr, float slope, long rows,
    int D, int H, int W, const double *__restrict__ sums, float *__restrict__ dx) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long row0 = ((long)blockIdx.x * WAVES + wave) * ROWS_PER_WAVE;
  const int nvec = W >> 2;
  for (int r = 0; r < ROWS_PER_WAVE; ++r) {
    const long row = row0 + r;   // (b c, d, h)
    if (row >= rows) break;
    const int h = (int)(row % H);
    const long t = row / H;
    const int d = (int)(t % D);
    const long bc = t / D;
    const float mu = mean[bc], rs = rstd[bc];
    const float m1 = (float)sums[2 * bc], m2 = (float)sums[2 * bc + 1];
    const float grd = GATED ? gr[(bc * H + h) * D + d] : 1.0f;
    auto cell = [&](float xv, float gv, float glv) __attribute__((always_inline)) {
      const float xh = (xv - mu) * rs;
      const float k = xh > 0.0f ? 1.0f : slope;
      const float u = GATED ? gv * (glv * grd) * k : gv * k;
      return rs * (u - m1 - xh * m2);
    };
    const float *xr = x + row * W, *gp = g + row * W;
    const float *glr = GATED ? gl + (bc * H + h) * W : nullptr;
    float *o = dx + row * W;
    for (int q = lane; q < nvec; q += 64) {
      const f32x4u xv = *reinterpret_cast<const f32x4u *>(xr + 4 * q);
      const f32x4u gv = *reinterpret_cast<const f32x4u *>(gp + 4 * q);
      f32x4u lv = {1.0f, 1.0f, 1.0f, 1.0f};
      if (GATED) lv = *reinterpret_cast<const f32x4u *>(glr + 4 * q);
      f32x4u out;
#pragma unroll
      for (int e = 0; e < 4; ++e) out[e] = cell(xv[e], gv[e], lv[e]);
      *reinterpret_cast<f32x4u *>(o + 4 * q) = out;
    }
    const int kt = 4 * nvec + lane;
    if (kt < W) o[kt] = cell(xr[kt], gp[kt], GATED ? glr[kt] : 1.0f);
  }
}

bool overlap(const float *a, const float *b, long n) { return a < b + n && b < a + n; }

// the shape rules every entry point shares; n = D H W cells per (b, c)
int check_shape(const char *who, int B, int C, int D, int H, int W) {
  SA_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0, "%s: bad shape B %d C %d D %d H %d W %d", who, B, C, D, H, W);
  const long n = (long)D * H * W;
  SA_REQUIRE(n < (1L << 30), "%s: bad shape (D*H*W = %ld must be below 2^30)", who, n);
  SA_REQUIRE(n > 1, "%s: bad shape (one cell per channel: InstanceNorm needs D*H*W > 1)", who);
  SA_REQUIRE((long)B * C * D * H <= 0x7fffffffL, "%s: bad shape (B*C*D*H = %ld rows exceed 2^31 - 1)", who,
             (long)B * C * D * H);
  return SA_OK;
}

long stat_parts(long n) { return (n + STAT_CHUNK - 1) / STAT_CHUNK; }

}  // namespace

extern "C" long sa_volume_close_stat_parts(int D, int H, int W) {
  if (D <= 0 || H <= 0 || W <= 0) return -1;
  return stat_parts((long)D * H * W);
}

extern "C" int sa_volume_close_stats(const float *x, int B, int C, int D, int H, int W, double *stats_partial,
                                     void *stream) {
  SA_REQUIRE(x && stats_partial, "sa_volume_close_stats: null pointer (x / stats_partial)");
  if (int rc = check_shape("sa_volume_close_stats", B, C, D, H, W)) return rc;
  const long n = (long)D * H * W, parts = stat_parts(n), blocks = (long)B * C * parts;
  SA_REQUIRE(blocks <= 0x7fffffffL, "sa_volume_close_stats: bad shape (%ld blocks exceed 2^31 - 1)", blocks);
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  close_stats_kernel<<<(unsigned)blocks, THREADS, 0, s>>>(x, n, (int)parts, stats_partial);
  return sa::check_launch("sa_volume_close_stats");
}

extern "C" long sa_volume_close_backward_work(int B, int C, int H) {
  if (B <= 0 || C <= 0 || H <= 0) return -1;
  return 2L * B * C * (H + 1);
}

extern "C" int sa_volume_close_backward(const float *x, const float *grad_out, int B, int C, int D, int H, int W,
                                        const float *mean, const float *rstd, const float *gate_l,
                                        const float *gate_r, float slope, double *work, float *grad_x,
                                        float *grad_gate_l, float *grad_gate_r, void *stream) {
  SA_REQUIRE(x && grad_out && mean && rstd && work,
             "sa_volume_close_backward: null pointer (x / grad_out / mean / rstd / work)");
  if (int rc = check_shape("sa_volume_close_backward", B, C, D, H, W)) return rc;
  SA_REQUIRE((gate_l == nullptr) == (gate_r == nullptr), "sa_volume_close_backward: gate_l and gate_r go together");
  SA_REQUIRE(gate_l || (!grad_gate_l && !grad_gate_r),
             "sa_volume_close_backward: grad_gate_l / grad_gate_r need the gate maps");
  SA_REQUIRE(grad_x || grad_gate_l || grad_gate_r,
             "sa_volume_close_backward: no output (grad_x, grad_gate_l and grad_gate_r are all null)");
  const long bc = (long)B * C, n = (long)D * H * W, rows = bc * D * H;
  if (grad_x)
    SA_REQUIRE(!overlap(grad_x, x, bc * n) && !overlap(grad_x, grad_out, bc * n),
               "sa_volume_close_backward: grad_x overlaps x or grad_out");
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  double *partial = grad_x ? work : nullptr, *sums = work + 2 * bc * H;
  const unsigned grid = (unsigned)(bc * H);
  if (gate_l) {
    close_bwd_reduce_kernel<true><<<grid, THREADS, 0, s>>>(x, grad_out, mean, rstd, gate_l, gate_r, slope, D, H, W,
                                                            partial, grad_gate_l, grad_gate_r);
  } else {
    close_bwd_reduce_kernel<false><<<grid, THREADS, 0, s>>>(x, grad_out, mean, rstd, nullptr, nullptr, slope, D, H, W,
                                                             partial, nullptr, nullptr);
  }
  if (grad_x) {
    close_bwd_fold_kernel<<<(unsigned)bc, 64, 0, s>>>(partial, H, (double)n, sums);
    const unsigned agrid = (unsigned)((rows + WAVES * ROWS_PER_WAVE - 1) / (WAVES * ROWS_PER_WAVE));
    if (gate_l) {
      close_bwd_apply_kernel<true><<<agrid, THREADS, 0, s>>>(x, grad_out, mean, rstd, gate_l, gate_r, slope, rows, D, H,
                                                             W, sums, grad_x);
    } else {
      close_bwd_apply_kernel<false><<<agrid, THREADS, 0, s>>>(x, grad_out, mean, rstd, nullptr, nullptr, slope, rows, D,
                                                              H, W, sums, grad_x);
    }
  }
  return sa::check_launch("sa_volume_close_backward");
}

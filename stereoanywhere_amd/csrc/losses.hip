// The fused training loss of train.py:281-379: the L1, normals and confidence-BCE terms of K maps
// against one ground truth, forward and backward.  The semantics (formulas, NaN rules, the record)
// are in stereoanywhere_hip.h; this file is their kernels.
//
// Data is fp32; every element's arithmetic is fp64 and each output is rounded once (the yardstick
// of tests/test_gpu_losses.py is 4 x the reference formulation's own fp32 error, and a term is one
// scalar: only a correctly rounded result is below that whatever the roundings of the fp32
// formulation happen to be, as in lsq_backward.hip).  The work is bound by the maps' traffic, not by
// the fp64 rate.  Deterministic: no floating-point atomics, fixed summation orders.
//
// The maps of one launch (SA_LOSS_MAX_MAPS at most) travel by value in the kernel arguments.
//   loss_stats_kernel     grid (SPLIT, B, maps): min / max / NaN flag of sign * map over a slice of a
//                         plane, for the maps whose normals term or skip-if-NaN flag needs them
//   loss_fwd_kernel       grid (W / 64, H / 16, B): a block owns a 64 x 16 tile, four pixels a thread;
//                         gt, valid, the selection bits and the target normals are fetched once and
//                         kept in registers while the block walks the maps.  Per map: the lane tree,
//                         lane 63 of each wave into its own LDS slot; after the last map the four
//                         waves are added in order and the block writes its partial sums
//   loss_finalise_kernel  one block: a wave per row of partial sums in block order, then a thread
//                         per map applies the drop / propagate rules, and thread 0 adds the total
//   loss_bwd_kernel       grid (W / 64, H / 4, B): a thread per pixel recomputes the forward around its
//                         pixel from the inputs and the record and writes every requested gradient
#include <cmath>
#include <cstdint>

#include "sa_common.h"

namespace {

constexpr int MAXK = SA_LOSS_MAX_MAPS;
constexpr int TW = 64, TH = 16, PPT = 4;   // forward tile; PPT rows a thread, 4 apart
constexpr int BTH = 4;                     // backward tile: 64 x 4
constexpr int SPLIT = 8;                   // slices of a plane in loss_stats_kernel
constexpr int KMAX_TOTAL = 4096;
constexpr double EPS = 1e-4;               // normalize()'s eps

struct DevMaps {
  int n, k0;   // maps in this launch; index of the first among all K
  SaLossMap m[MAXK];
};

__device__ __forceinline__ bool needs_stats(const SaLossMap &M) {
  return M.w_n != 0.0 || (M.flags & SA_LOSS_SKIP_IF_NAN_MAP);
}

// bit 0: mask; bit 1: mask and border
__device__ __forceinline__ int sel_bits(float gt, float valid, int x, int W, double maxdisp, int border) {
  if (!(valid > 0.0f && (double)gt < maxdisp)) return 0;
  bool in = true;
  if (border == SA_LOSS_BORDER_LEFT) in = (double)x - (double)gt >= 0.0;
  if (border == SA_LOSS_BORDER_RIGHT) in = (double)x + (double)gt < (double)W;
  return in ? 3 : 1;
}

__device__ __forceinline__ double softplus64(double z) { return z > 20.0 ? z : log1p(exp(z)); }

// The BCE target of a pixel: clip(softplus(th - |m - gt|) / div, 0, 1); NaN stays NaN.
__device__ __forceinline__ double bce_target(float m, float gt, double th, double div) {
  const double t = softplus64(th - fabs((double)m - (double)gt)) / div;
  return t != t ? t : fmin(fmax(t, 0.0), 1.0);
}

// ------------------------------------------------------------------------------------ stats
__global__ __launch_bounds__(256) void loss_stats_kernel(DevMaps P, int B, long hw, float *__restrict__ stats) {
  const SaLossMap &M = P.m[blockIdx.z];
  if (!needs_stats(M)) return;   // block-uniform: nothing reads this map's slots
  __shared__ float red[4][3];
  const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  const long chunk = (hw + SPLIT - 1) / SPLIT;
  const long lo = (long)s * chunk, hi = lo + chunk < hw ? lo + chunk : hw;
  const float *p = M.map + (long)b * hw;
  const float sg = (float)M.sign;
  float mn = INFINITY, mx = -INFINITY;
  bool nan = false;
  for (long i = lo + tid; i < hi; i += 4 * 256) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long j = i + u * 256;
      if (j < hi) {
        const float v = sg * p[j];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
        nan |= v != v;
      }
    }
  }
  mx = sa::wave_max_dpp(mx);
  mn = -sa::wave_max_dpp(-mn);
  const bool any = __ballot(nan) != 0;
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = mn;
    red[tid >> 6][1] = mx;
    red[tid >> 6][2] = any ? 1.0f : 0.0f;
  }
  __syncthreads();
  if (tid == 0) {
    float *o = stats + (((long)(P.k0 + blockIdx.z) * B + b) * SPLIT + s) * 4;
    o[0] = fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0]));
    o[1] = fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1]));
    o[2] = red[0][2] + red[1][2] + red[2][2] + red[3][2];
  }
}

// mn, mx and the NaN flag of (map k, sample b) from the SPLIT slices (an empty slice holds +-inf, 0)
__device__ __forceinline__ void plane_stats(const float *__restrict__ stats, int k, int B, int b, float &mn, float &mx,
                                            bool &nan) {
  const float *o = stats + ((long)k * B + b) * SPLIT * 4;
  mn = INFINITY, mx = -INFINITY, nan = false;
#pragma unroll
  for (int s = 0; s < SPLIT; ++s) {
    mn = fminf(mn, o[4 * s]);
    mx = fmaxf(mx, o[4 * s + 1]);
    nan |= o[4 * s + 2] != 0.0f;
  }
}

// One pixel's normal (a, b, 1) before its normalisation, from the map around (y, x): g = gain z.
struct NormalAB {
  double a, b;
};
__device__ __forceinline__ NormalAB normal_ab(const float *__restrict__ plane, int H, int W, int y, int x, double sg,
                                              double mn, double den, double gain) {
  const int xl = x > 0 ? x - 1 : 0, xr = x < W - 1 ? x + 1 : W - 1;
  const int yu = y > 0 ? y - 1 : 0, yd = y < H - 1 ? y + 1 : H - 1;
  const long row = (long)y * W;
  auto g = [&](long i) { return gain * ((sg * (double)plane[i] - mn) / den); };
  NormalAB r;
  r.a = -(g(row + xr) - g(row + xl));
  r.b = -(g((long)yd * W + x) - g((long)yu * W + x));
  return r;
}

// ---------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(256) void loss_fwd_kernel(DevMaps P, const float *__restrict__ gt,
                                                       const float *__restrict__ valid,
                                                       const float *__restrict__ target, int B, int H, int W,
                                                       double maxdisp, int border, double gain, double lrc_th,
                                                       double div, const float *__restrict__ stats,
                                                       double *__restrict__ partial, long nblocks, int counts) {
  __shared__ double red[4][MAXK][4];
  __shared__ double cnt[4][2];
  const int tid = threadIdx.x, tx = tid & 63, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.z;
  const long blk = ((long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const long hw = (long)H * W;
  const int x = blockIdx.x * TW + tx;
  int ys[PPT], bits[PPT];
  float gtv[PPT], t0[PPT], t1[PPT], t2[PPT];
  double cm = 0.0, cb = 0.0;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    ys[j] = blockIdx.y * TH + wave + 4 * j;
    bits[j] = 0;
    gtv[j] = t0[j] = t1[j] = t2[j] = 0.0f;
    if (x < W && ys[j] < H) {
      const long q = (long)ys[j] * W + x;
      gtv[j] = gt[b * hw + q];
      bits[j] = sel_bits(gtv[j], valid[b * hw + q], x, W, maxdisp, border);
      if (target) {
        t0[j] = target[(3L * b) * hw + q];
        t1[j] = target[(3L * b + 1) * hw + q];
        t2[j] = target[(3L * b + 2) * hw + q];
      }
      cm += bits[j] & 1;
      cb += (bits[j] >> 1) & 1;
    }
  }
  cm = sa::wave_sum_dpp_lane63(cm);
  cb = sa::wave_sum_dpp_lane63(cb);
  if (lane == 63) cnt[wave][0] = cm, cnt[wave][1] = cb;

  for (int k = 0; k < P.n; ++k) {
    const SaLossMap &M = P.m[k];
    const float *plane = M.map + b * hw;
    const int need = M.sel == SA_LOSS_SEL_MASK_BORDER ? 2 : 1;
    const double sg = (double)M.sign;
    double mn = 0.0, den = 1.0;
    if (M.w_n != 0.0) {
      float fmn, fmx;
      bool nan;
      plane_stats(stats, P.k0 + k, B, b, fmn, fmx, nan);
      mn = (double)fmn;
      den = ((double)fmx - (double)fmn) + EPS;
    }
    double s_l1 = 0.0, s_n = 0.0, s_b = 0.0, n_b = 0.0;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      if (!bits[j]) continue;   // outside the plane or the mask: in no selection
      const long q = (long)ys[j] * W + x;
      const float m = plane[q];
      if (bits[j] & need) {
        if (M.w_l1 != 0.0) s_l1 += fabs(sg * (double)m - (double)gtv[j]);
        if (M.w_n != 0.0) {
          const NormalAB n = normal_ab(plane, H, W, ys[j], x, sg, mn, den, gain);
          const double nrm = sqrt(n.a * n.a + n.b * n.b + 1.0);
          s_n += 1.0 - (n.a * (double)t0[j] + n.b * (double)t1[j] + (double)t2[j]) / nrm;
        }
      }
      if (M.w_bce != 0.0) {
        const float c = M.conf[b * hw + q];
        const double tg = bce_target(m, gtv[j], lrc_th, div);
        if (c == c && tg == tg) {
          const double cc = fmin(fmax((double)c, 0.0), 1.0);
          s_b += -(tg * fmax(log(cc), -100.0) + (1.0 - tg) * fmax(log(1.0 - cc), -100.0));
          n_b += 1.0;
        }
      }
    }
    s_l1 = sa::wave_sum_dpp_lane63(s_l1);
    s_n = sa::wave_sum_dpp_lane63(s_n);
    s_b = sa::wave_sum_dpp_lane63(s_b);
    n_b = sa::wave_sum_dpp_lane63(n_b);
    if (lane == 63) red[wave][k][0] = s_l1, red[wave][k][1] = s_n, red[wave][k][2] = s_b, red[wave][k][3] = n_b;
  }
  __syncthreads();
  for (int i = tid; i < 4 * P.n; i += 256) {
    const int k = i >> 2, j = i & 3;
    partial[(2 + 4L * (P.k0 + k) + j) * nblocks + blk] = ((red[0][k][j] + red[1][k][j]) + red[2][k][j]) + red[3][k][j];
  }
  if (counts && tid < 2) partial[tid * nblocks + blk] = ((cnt[0][tid] + cnt[1][tid]) + cnt[2][tid]) + cnt[3][tid];
}

// --------------------------------------------------------------------------------- finalise
__global__ __launch_bounds__(1024) void loss_finalise_kernel(DevMaps P, int K, int B, const float *__restrict__ stats,
                                                             const double *__restrict__ partial, long nblocks,
                                                             double *__restrict__ rec, float *__restrict__ out) {
  __shared__ double sums[4 * MAXK + 2];
  __shared__ double contrib[MAXK];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nrows = 4 * P.n + 2;
  for (int r = wave; r < nrows; r += 16) {   // wave-uniform
    const double *row = partial + (r < 2 ? (long)r : 2 + 4L * P.k0 + (r - 2)) * nblocks;
    double acc = 0.0;
    for (long i = lane; i < nblocks; i += 64) acc += row[i];
    acc = sa::wave_sum_dpp_lane63(acc);
    if (lane == 63) sums[r] = acc;
  }
  __syncthreads();
  if (tid < P.n) {
    const SaLossMap &M = P.m[tid];
    const int k = P.k0 + tid;
    double *R = rec + 4 + 8L * k, *mm = rec + 4 + 8L * K + 2L * k * B;
    bool nanmap = false;
    for (int b = 0; b < B; ++b) {
      float mn = 0.0f, mx = 0.0f;
      bool nan = false;
      if (needs_stats(M)) plane_stats(stats, k, B, b, mn, mx, nan);
      mm[2 * b] = (double)mn;
      mm[2 * b + 1] = (double)mx;
      nanmap |= nan;
    }
    const bool skipped = (M.flags & SA_LOSS_SKIP_IF_NAN_MAP) && nanmap;
    const double count = sums[M.sel == SA_LOSS_SEL_MASK_BORDER ? 1 : 0];
    const double *S = sums + 2 + 4 * tid;
    const double term[3] = {S[0] / count, nanmap ? (double)NAN : S[1] / count, S[2] / S[3]};
    const double w[3] = {M.w_l1, M.w_n, M.w_bce};
    const double cnts[3] = {count, count, S[3]};
    const bool drop[3] = {(M.flags & SA_LOSS_DROP_NAN_L1) != 0, true, (M.flags & SA_LOSS_DROP_NAN_BCE) != 0};
    double add = 0.0;
    for (int j = 0; j < 3; ++j) {
      const bool on = w[j] != 0.0 && !skipped;
      const bool live = on && !(drop[j] && term[j] != term[j]);
      if (live) add += w[j] * term[j];
      R[1 + j] = live ? w[j] / cnts[j] : 0.0;
      R[4 + j] = on ? term[j] : 0.0;
      out[1 + 3 * k + j] = on ? (float)term[j] : 0.0f;
    }
    R[0] = skipped ? 1.0 : 0.0;
    R[7] = S[3];
    contrib[tid] = add;
  }
  __syncthreads();
  if (tid == 0) {
    double total = P.k0 ? rec[0] : 0.0;
    for (int k = 0; k < P.n; ++k) total += contrib[k];
    rec[0] = total;
    rec[1] = total != total ? 1.0 : 0.0;
    rec[2] = sums[0];
    rec[3] = sums[1];
    out[0] = (float)total;
  }
}

// --------------------------------------------------------------------------------- backward
// d (1 - n . t) / d a and / d b at pixel (y, x) of a map
__device__ __forceinline__ NormalAB normal_grad(const float *__restrict__ plane, int H, int W, int y, int x, double sg,
                                                double mn, double den, double gain, double t0, double t1, double t2) {
  const NormalAB n = normal_ab(plane, H, W, y, x, sg, mn, den, gain);
  const double q = n.a * n.a + n.b * n.b + 1.0, nrm = sqrt(q);
  const double dot = n.a * t0 + n.b * t1 + t2;
  NormalAB r;
  r.a = -(t0 / nrm - dot * n.a / (q * nrm));
  r.b = -(t1 / nrm - dot * n.b / (q * nrm));
  return r;
}

struct Tap {   // a pixel whose normal reads this thread's pixel: its position, selection bits and target
  int y, x, bits;
  float t0, t1, t2;
};

__global__ __launch_bounds__(256) void loss_bwd_kernel(DevMaps P, const float *__restrict__ gt,
                                                       const float *__restrict__ valid,
                                                       const float *__restrict__ target, int K, int B, int H, int W,
                                                       double maxdisp, int border, double gain, double lrc_th,
                                                       double div, const double *__restrict__ rec,
                                                       const float *__restrict__ g_total) {
  const int x = blockIdx.x * TW + (threadIdx.x & 63), y = blockIdx.y * BTH + (threadIdx.x >> 6), b = blockIdx.z;
  if (x >= W || y >= H) return;
  const long hw = (long)H * W, q = (long)y * W + x;
  const double up = rec[1] != 0.0 ? 0.0 : (double)g_total[0];   // a NaN total: zeros
  const float gtq = gt[b * hw + q];
  const int bq = sel_bits(gtq, valid[b * hw + q], x, W, maxdisp, border);
  // the taps of the stencil's adjoint in their fixed order: (y, x-1), (y, x), (y, x+1) read this pixel
  // through a, (y-1, x), (y, x), (y+1, x) through b; the pixel itself only where an index clamps
  Tap tap[5];
  if (target) {
    const int ty[5] = {y, y, y, y > 0 ? y - 1 : 0, y < H - 1 ? y + 1 : H - 1};
    const int tx[5] = {x > 0 ? x - 1 : 0, x, x < W - 1 ? x + 1 : W - 1, x, x};
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const long p = (long)ty[i] * W + tx[i];
      tap[i].y = ty[i], tap[i].x = tx[i];
      tap[i].bits = sel_bits(gt[b * hw + p], valid[b * hw + p], tx[i], W, maxdisp, border);
      tap[i].t0 = target[(3L * b) * hw + p];
      tap[i].t1 = target[(3L * b + 1) * hw + p];
      tap[i].t2 = target[(3L * b + 2) * hw + p];
    }
  }
  for (int k = 0; k < P.n; ++k) {
    const SaLossMap &M = P.m[k];
    if (!M.grad_map && !M.grad_conf) continue;
    const double *R = rec + 4 + 8L * (P.k0 + k);
    const double c_l1 = up * R[1], c_n = up * R[2], c_b = up * R[3];
    const float *plane = M.map + b * hw;
    const float m = plane[q];
    const int need = M.sel == SA_LOSS_SEL_MASK_BORDER ? 2 : 1;
    const double sg = (double)M.sign;
    if (M.grad_map) {
      double g = 0.0;
      if (c_l1 != 0.0 && (bq & need)) {
        const double d = sg * (double)m - (double)gtq;
        g = c_l1 * (d > 0.0 ? sg : (d < 0.0 ? -sg : 0.0));
      }
      if (c_n != 0.0 && target) {
        const double *mm = rec + 4 + 8L * K + 2L * ((long)(P.k0 + k) * B + b);
        const double mn = mm[0], den = (mm[1] - mm[0]) + EPS;
        auto grad = [&](const Tap &t) {
          if (!(t.bits & need)) return NormalAB{0.0, 0.0};
          return normal_grad(plane, H, W, t.y, t.x, sg, mn, den, gain, (double)t.t0, (double)t.t1, (double)t.t2);
        };
        const NormalAB self = grad(tap[1]);
        double acc = 0.0;
        if (x > 0) acc -= grad(tap[0]).a;
        if (x == W - 1) acc -= self.a;
        if (x == 0) acc += self.a;
        if (x < W - 1) acc += grad(tap[2]).a;
        if (y > 0) acc -= grad(tap[3]).b;
        if (y == H - 1) acc -= self.b;
        if (y == 0) acc += self.b;
        if (y < H - 1) acc += grad(tap[4]).b;
        g += sg * (c_n * (acc * (gain / den)));
      }
      M.grad_map[b * hw + q] = (float)g;
    }
    if (M.grad_conf) {
      double g = 0.0;
      if (c_b != 0.0 && (bq & 1) && M.conf) {
        const float c = M.conf[b * hw + q];
        const double tg = bce_target(m, gtq, lrc_th, div);
        if (c == c && tg == tg && c > 0.0f && c < 1.0f) {
          const double cc = (double)c;
          const double dl = log(cc) > -100.0 ? 1.0 / cc : 0.0, dr = log(1.0 - cc) > -100.0 ? 1.0 / (1.0 - cc) : 0.0;
          g = c_b * ((1.0 - tg) * dr - tg * dl);
        }
      }
      M.grad_conf[b * hw + q] = (float)g;
    }
  }
}

long tiles(int H, int W) { return (long)((W + TW - 1) / TW) * ((H + TH - 1) / TH); }
bool shape_ok(int K, int B, int H, int W) {
  return K >= 1 && K <= KMAX_TOTAL && B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long)H * W < (1L << 31) &&
         (H + BTH - 1) / BTH <= 65535;
}
long partial_doubles(int K, int B, int H, int W) { return (2 + 4L * K) * (tiles(H, W) * B); }

int check_args(const char *who, int K, const SaLossMap *maps, const float *gt, const float *valid, const float *target,
               int B, int H, int W, int border_mode, const void *rec) {
  SA_REQUIRE(K >= 1 && K <= KMAX_TOTAL, "%s: K must be 1..%d, got %d", who, KMAX_TOTAL, K);
  SA_REQUIRE(maps && gt && valid && rec, "%s: null pointer (maps / gt / valid / rec)", who);
  SA_REQUIRE(shape_ok(K, B, H, W), "%s: bad shape (B %d, H %d, W %d)", who, B, H, W);
  SA_REQUIRE(border_mode >= SA_LOSS_BORDER_NONE && border_mode <= SA_LOSS_BORDER_RIGHT,
             "%s: border_mode must be 0 (none), 1 (left) or 2 (right), got %d", who, border_mode);
  SA_REQUIRE((reinterpret_cast<uintptr_t>(rec) & 7) == 0, "%s: rec not 8-byte aligned", who);
  for (int k = 0; k < K; ++k) {
    const SaLossMap &M = maps[k];
    SA_REQUIRE(M.map, "%s: null pointer (map %d)", who, k);
    SA_REQUIRE(M.sign == 1 || M.sign == -1, "%s: map %d: sign must be -1 or +1, got %d", who, k, M.sign);
    SA_REQUIRE(M.sel == SA_LOSS_SEL_MASK || M.sel == SA_LOSS_SEL_MASK_BORDER,
               "%s: map %d: sel must be 0 (mask) or 1 (mask and border), got %d", who, k, M.sel);
    SA_REQUIRE((M.flags & ~7) == 0, "%s: map %d: unknown flags %d", who, k, M.flags);
    SA_REQUIRE(M.w_l1 == M.w_l1 && M.w_n == M.w_n && M.w_bce == M.w_bce, "%s: map %d: a weight is NaN", who, k);
    SA_REQUIRE(M.w_n == 0.0 || target, "%s: map %d has a normals weight but target is null", who, k);
    SA_REQUIRE(M.w_bce == 0.0 || M.conf, "%s: map %d has a BCE weight but no confidence", who, k);
  }
  return SA_OK;
}

DevMaps pack(const SaLossMap *maps, int k0, int K) {
  DevMaps P;
  P.k0 = k0;
  P.n = K - k0 < MAXK ? K - k0 : MAXK;
  for (int i = 0; i < MAXK; ++i) P.m[i] = maps[k0 + (i < P.n ? i : 0)];
  return P;
}

}  // namespace

extern "C" long sa_loss_terms_ws_size(int K, int B, int H, int W) {
  if (!shape_ok(K, B, H, W)) return -1;
  return partial_doubles(K, B, H, W) * (long)sizeof(double) + (long)K * B * SPLIT * 4 * (long)sizeof(float);
}

extern "C" long sa_loss_terms_rec_size(int K, int B) {
  if (K < 1 || K > KMAX_TOTAL || B < 1 || B > 65535) return -1;
  return (4 + 8L * K + 2L * K * B) * (long)sizeof(double);
}

extern "C" int sa_loss_terms_forward(int K, const SaLossMap *maps, const float *gt, const float *valid,
                                     const float *target, int B, int H, int W, double maxdisp, int border_mode,
                                     double gain, double lrc_th, void *ws, double *rec, float *out, void *stream) {
  int rc = check_args("sa_loss_terms_forward", K, maps, gt, valid, target, B, H, W, border_mode, rec);
  if (rc) return rc;
  SA_REQUIRE(ws && out, "sa_loss_terms_forward: null pointer (ws / out)");
  SA_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "sa_loss_terms_forward: workspace not 8-byte aligned");
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  const long nblocks = tiles(H, W) * B, hw = (long)H * W;
  double *partial = static_cast<double *>(ws);
  float *stats = reinterpret_cast<float *>(partial + partial_doubles(K, B, H, W));
  const double div = std::log(1.0 + std::exp(lrc_th));
  const dim3 grid((unsigned)((W + TW - 1) / TW), (unsigned)((H + TH - 1) / TH), (unsigned)B);
  for (int k0 = 0; k0 < K; k0 += MAXK) {
    const DevMaps P = pack(maps, k0, K);
    bool any = false;
    for (int i = 0; i < P.n; ++i) any |= P.m[i].w_n != 0.0 || (P.m[i].flags & SA_LOSS_SKIP_IF_NAN_MAP);
    if (any) {
      loss_stats_kernel<<<dim3(SPLIT, (unsigned)B, (unsigned)P.n), 256, 0, s>>>(P, B, hw, stats);
      if ((rc = sa::check_launch("sa_loss_terms_forward/stats"))) return rc;
    }
    loss_fwd_kernel<<<grid, 256, 0, s>>>(P, gt, valid, target, B, H, W, maxdisp, border_mode, gain, lrc_th, div, stats,
                                         partial, nblocks, k0 == 0);
    if ((rc = sa::check_launch("sa_loss_terms_forward/sums"))) return rc;
    loss_finalise_kernel<<<1, 1024, 0, s>>>(P, K, B, stats, partial, nblocks, rec, out);
    if ((rc = sa::check_launch("sa_loss_terms_forward/finalise"))) return rc;
  }
  return SA_OK;
}

extern "C" int sa_loss_terms_backward(int K, const SaLossMap *maps, const float *gt, const float *valid,
                                      const float *target, int B, int H, int W, double maxdisp, int border_mode,
                                      double gain, double lrc_th, const double *rec, const float *g_total,
                                      void *stream) {
  int rc = check_args("sa_loss_terms_backward", K, maps, gt, valid, target, B, H, W, border_mode, rec);
  if (rc) return rc;
  SA_REQUIRE(g_total, "sa_loss_terms_backward: null pointer (g_total)");
  bool any = false;
  for (int k = 0; k < K; ++k) {
    any |= maps[k].grad_map || maps[k].grad_conf;
    SA_REQUIRE(!maps[k].grad_conf || maps[k].conf, "sa_loss_terms_backward: map %d: grad_conf requested without conf", k);
  }
  SA_REQUIRE(any, "sa_loss_terms_backward: null pointer (no gradient requested)");
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  const double div = std::log(1.0 + std::exp(lrc_th));
  const dim3 grid((unsigned)((W + TW - 1) / TW), (unsigned)((H + BTH - 1) / BTH), (unsigned)B);
  for (int k0 = 0; k0 < K; k0 += MAXK) {
    const DevMaps P = pack(maps, k0, K);
    bool some = false;
    for (int i = 0; i < P.n; ++i) some |= P.m[i].grad_map || P.m[i].grad_conf;
    if (!some) continue;
    loss_bwd_kernel<<<grid, 256, 0, s>>>(P, gt, valid, target, K, B, H, W, maxdisp, border_mode, gain, lrc_th, div, rec,
                                         g_total);
    if ((rc = sa::check_launch("sa_loss_terms_backward"))) return rc;
  }
  return SA_OK;
}

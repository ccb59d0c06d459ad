// Backward of the mono-scale alignment ops on the reference's fine-tuning gradient path: softLRC
// with its fused confidence product (lsq.hip softlrc_kernel; utils.py:172-198, 240-241) and
// weighted_lsq (lsq_select.h lsq1_kernel; utils.py:345-384).  The formulas are in stereoanywhere_hip.h.
//
// Data is fp32; the arithmetic between the loads and the one rounding of each output element is
// fp64.  The reason is the yardstick of tests/test_gpu_lsq_lrc_backward.py (4 x the reference
// formulation's own fp32 error e_ref): on a plane of a few pixels e_ref is the rounding of a handful
// of results, and only a correctly rounded gradient is below it element by element whatever those
// roundings are.  (An fp32 version was not measured against it.)  Both ops are small (a map of B H W
// pixels, no reduction axis), so the fp64 rate is not what bounds them.  Deterministic: no
// floating-point atomics, one fixed summation order per element.
//
// softLRC.  The forward's warp is a scatter in the backward's direction: pixel p of one map reads up
// to four taps of the other map at a column that depends on p's own disparity.  Two launches, both
// maps in each (blockIdx.y):
//   lrcb_px_kernel — one thread per pixel recomputes the forward: the cell (floor, bounds) from the
//     forward's own fp32 arithmetic (lrc_sample.h), so that both pick the same taps, the weights
//     within that cell in fp64.  It writes grad_conf, t = d loss / d u into the workspace, and the
//     pixel's own term of grad_d (direct + coordinate) either as the result (nothing samples that
//     map) or into the workspace;
//   lrcb_gather_kernel — one thread per target pixel (y, x) of the sampled map scans the source rows
//     whose tap rows include y (iy = y' (H - 1) / H floors to y' - 1 or y', so y' in y - 1 .. y + 1; a
//     row is skipped as a whole when neither of its two tap rows is y), recomputes each source
//     pixel's column cell and adds -t weight where a tap is (y, x): ascending in source row, then
//     column, into one accumulator, adds the own term and rounds once.  O(W) per pixel.
//
// weighted_lsq.  lsqb_kernel is element-wise: every thread solves its sample's 2x2 system from the
// record sa_weighted_lsq_stats left (lsq_stats.hip: the forward kernel's second instance) and forms its
// element's three gradients.
#include <cmath>
#include <cstdint>

#include "lrc_sample.h"
#include "sa_common.h"

namespace {

// ------------------------------------------------------------------------------------ softLRC
// One map's side of the forward: s = softlrc(dself; dother warped by relu(dself)) * conf.
struct LrcSide {
  const float *dself, *dother, *conf, *g;   // conf null: no product; g null: this output was not used
  float *grad_d, *grad_conf;                // null: not requested, or (grad_d) finished by the gather
  double *own, *t;                          // workspace maps [B,H,W]: the own term of grad_d for the gather; t
  float sign;                               // -1: left map, +1: right map
};

// the fp64 source column of pixel x with relu'd disparity r (ix = ((x -+ r) / W) (W - 1))
__device__ __forceinline__ double lrc_ix64(int x, float r, float sign, double kx) {
  return (sign < 0 ? (double)x - (double)r : (double)x + (double)r) * kx;
}

__global__ __launch_bounds__(256) void lrcb_px_kernel(LrcSide s0, LrcSide s1, int H, int W, long bs, float th,
                                                      double div, long npix) {
  const LrcSide S = blockIdx.y ? s1 : s0;
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const long hw = (long)H * W;
  const long b = p / hw, r = p % hw;
  const long o = b * bs + r;
  if (!S.g) {   // (block-uniform) no upstream gradient: the own terms are 0, nothing to scatter
    if (S.grad_d) S.grad_d[o] = 0.0f;
    if (S.own) S.own[p] = 0.0;
    if (S.grad_conf) S.grad_conf[o] = 0.0f;
    return;
  }
  const int y = (int)(r / W), x = (int)(r % W);
  const float *a = S.dself + b * bs, *c = S.dother + b * bs;
  const float d = a[r];
  float gx, gy;
  sa::lrc_grid(H, W, y, x, fmaxf(d, 0.0f), S.sign, gx, gy);
  const sa::LrcTaps T = sa::lrc_taps(H, W, gx, gy);   // the forward's cell
  auto at = [&](int yy, int xx) { return sa::lrc_inside(H, W, yy, xx) ? (double)c[(long)yy * W + xx] : 0.0; };
  const double v00 = at(T.yi, T.xi), v01 = at(T.yi, T.xi + 1), v10 = at(T.yi + 1, T.xi), v11 = at(T.yi + 1, T.xi + 1);
  // the weights within that cell (a cell clamped far outside the plane has no tap inside: all v are 0)
  const double kx = (double)(W - 1) / (double)W, ky = (double)(H - 1) / (double)H;
  const double w = lrc_ix64(x, fmaxf(d, 0.0f), S.sign, kx) - (double)T.xi, e = 1.0 - w;
  const double n = (double)y * ky - (double)T.yi, s = 1.0 - n;
  const double warped = v00 * (s * e) + v01 * (s * w) + v10 * (n * e) + v11 * (n * w);
  const double u = (double)d - warped;
  const double z = (double)th - fabs(u);
  const double g = (double)S.g[o];
  if (S.grad_conf) S.grad_conf[o] = (float)(g * ((z > 20.0 ? z : log1p(exp(z))) / div));
  const double slope = z > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-z));   // softplus'
  const double sgn = u > 0.0 ? 1.0 : (u < 0.0 ? -1.0 : 0.0);
  const double gc = S.conf ? g * (double)S.conf[o] : g;
  const double t = gc * (-(slope * sgn) / div);
  if (S.t) S.t[p] = t;
  if (S.grad_d || S.own) {
    // du/dd = 1 - dS/dix dix/dd, dix/dd = sign (W - 1) / W where d > 0; a tap outside the plane is 0
    const double dS = (v01 - v00) * s + (v11 - v10) * n;
    const double dix = d > 0.0f ? (double)S.sign * kx : 0.0;
    const double own = t * (1.0 - dS * dix);
    if (S.grad_d) S.grad_d[o] = (float)own;
    if (S.own) S.own[p] = own;
  }
}

// grad (the sampled map's gradient) = its own term + the tap terms of the pixels of the map that
// sampled it: dsrc that map's disparities, t its workspace map, sign its side.
struct LrcGather {
  const float *dsrc;
  const double *t, *own;
  float *grad;   // null: nothing to do
  float sign;
};

__global__ __launch_bounds__(256) void lrcb_gather_kernel(LrcGather j0, LrcGather j1, int H, int W, long bs,
                                                          long npix) {
  const LrcGather J = blockIdx.y ? j1 : j0;
  if (!J.grad) return;   // block-uniform
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const long hw = (long)H * W;
  const long b = p / hw, r = p % hw;
  const int yq = (int)(r / W), xq = (int)(r % W);
  const float *src = J.dsrc + b * bs;
  const double *tt = J.t + b * hw;
  const double kx = (double)(W - 1) / (double)W, ky = (double)(H - 1) / (double)H;
  double acc = 0.0;
  for (int y = max(0, yq - 1); y <= min(H - 1, yq + 1); ++y) {
    float gx, gy;
    sa::lrc_grid(H, W, y, 0, 0.0f, J.sign, gx, gy);
    const sa::LrcTaps R = sa::lrc_taps(H, W, gx, gy);   // (the row taps do not depend on x)
    if (R.yi != yq && R.yi + 1 != yq) continue;
    const double n = (double)y * ky - (double)R.yi;
    const double wy = R.yi == yq ? 1.0 - n : n;
    const float *srow = src + (long)y * W;
    const double *trow = tt + (long)y * W;
#pragma unroll 4
    for (int x = 0; x < W; ++x) {
      const float rd = fmaxf(srow[x], 0.0f);
      sa::lrc_grid(H, W, y, x, rd, J.sign, gx, gy);
      const sa::LrcTaps T = sa::lrc_taps(H, W, gx, gy);
      if (T.xi == xq || T.xi + 1 == xq) {
        const double w = lrc_ix64(x, rd, J.sign, kx) - (double)T.xi;
        acc += -trow[x] * (wy * (T.xi == xq ? 1.0 - w : w));
      }
    }
  }
  J.grad[b * bs + r] = (float)(J.own[p] + acc);
}

// ------------------------------------------------------------------------------- weighted LSQ
__global__ __launch_bounds__(256) void lsqb_kernel(const float *__restrict__ mde, const float *__restrict__ disp,
                                                   const float *__restrict__ conf, int n,
                                                   const float *__restrict__ scale, const float *__restrict__ shift,
                                                   const double *__restrict__ rec, const float *__restrict__ g_scale,
                                                   const float *__restrict__ g_shift, float *__restrict__ grad_mde,
                                                   float *__restrict__ grad_disp, float *__restrict__ grad_conf) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long o = (long)b * n + i;
  const double *rc = rec + (long)b * SA_LSQ_REC;
  float gm = 0.0f, gd = 0.0f, gc = 0.0f;
  if (rc[5] == 0.0) {   // full rank; the rank-deficient and the empty branch get zeros
    const double s11 = rc[0], s12 = rc[1], s22 = rc[2];
    const float lo = (float)rc[3], hi = (float)rc[4];
    const float m = mde[o], d = disp[o], c = conf[o];
    const float y = fmaxf(d, 0.0f);
    if (lo <= y && y <= hi) {
      const double g0 = g_scale ? (double)g_scale[b] : 0.0, g1 = g_shift ? (double)g_shift[b] : 0.0;
      const double det = s11 * s22 - s12 * s12;
      const double v0 = (s22 * g0 - s12 * g1) / det, v1 = (s11 * g1 - s12 * g0) / det;
      const double x0 = (double)scale[b], x1 = (double)shift[b];
      const double a = fabs((double)m), wt = fabs((double)c) * 0.9 + 0.1;
      const double u = a * v0 + v1;
      const double res = (double)y - (a * x0 + x1);
      const double sm = m > 0.0f ? 1.0 : (m < 0.0f ? -1.0 : 0.0);
      const double sc = c > 0.0f ? 1.0 : (c < 0.0f ? -1.0 : 0.0);
      gd = d > 0.0f ? (float)(wt * u) : 0.0f;
      gc = (float)(0.9 * sc * (u * res));
      gm = (float)(sm * (wt * (v0 * res - u * x0)));
    }
  }
  if (grad_mde) grad_mde[o] = gm;
  if (grad_disp) grad_disp[o] = gd;
  if (grad_conf) grad_conf[o] = gc;
}

}  // namespace

extern "C" long sa_softlrc_backward_ws_size(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return -1;
  return 4L * B * H * W * (long)sizeof(double);
}

extern "C" int sa_softlrc_backward(const float *d2, const float *d3, const float *conf2, const float *conf3, int B,
                                   int H, int W, long map_bs, float lrc_th, const float *g_s2, const float *g_s3,
                                   float *grad_d2, float *grad_d3, float *grad_conf2, float *grad_conf3, void *ws,
                                   void *stream) {
  SA_REQUIRE(d2 && d3, "sa_softlrc_backward: null pointer (d2 / d3)");
  SA_REQUIRE(g_s2 || g_s3, "sa_softlrc_backward: null pointer (both upstream gradients)");
  SA_REQUIRE(grad_d2 || grad_d3 || grad_conf2 || grad_conf3, "sa_softlrc_backward: null pointer (all four outputs)");
  SA_REQUIRE(!grad_conf2 || conf2, "sa_softlrc_backward: grad_conf2 requested without conf2");
  SA_REQUIRE(!grad_conf3 || conf3, "sa_softlrc_backward: grad_conf3 requested without conf3");
  SA_REQUIRE(B > 0 && H > 0 && W > 0, "sa_softlrc_backward: empty shape");
  SA_REQUIRE(map_bs >= (long)H * W, "sa_softlrc_backward: map_bs too small");
  // a map's gradient is finished by the gather when the other map's output has a gradient
  const bool gather2 = grad_d2 && g_s3, gather3 = grad_d3 && g_s2;
  SA_REQUIRE(!(gather2 || gather3) || ws, "sa_softlrc_backward: null pointer (workspace, needed for grad_d2 / grad_d3)");
  SA_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "sa_softlrc_backward: workspace not 8-byte aligned");
  const long npix = (long)B * H * W;
  const double div = std::log(1.0 + std::exp((double)lrc_th));
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  double *w = static_cast<double *>(ws);   // [t2 | t3 | own2 | own3], npix doubles each
  // a side's t map is read by the other map's gather only
  const LrcSide s0{d2, d3, conf2, g_s2, gather2 ? nullptr : grad_d2, grad_conf2, gather2 ? w + 2 * npix : nullptr,
                   gather3 ? w : nullptr, -1.0f};
  const LrcSide s1{d3, d2, conf3, g_s3, gather3 ? nullptr : grad_d3, grad_conf3, gather3 ? w + 3 * npix : nullptr,
                   gather2 ? w + npix : nullptr, +1.0f};
  const dim3 grid((unsigned)((npix + 255) / 256), 2);
  lrcb_px_kernel<<<grid, 256, 0, s>>>(s0, s1, H, W, map_bs, lrc_th, div, npix);
  int rc = sa::check_launch("sa_softlrc_backward/px");
  if (rc || !(gather2 || gather3)) return rc;
  // grad_d2 gathers from the right map's pixels (they sampled d2), grad_d3 from the left map's
  const LrcGather j0{d3, w + npix, w + 2 * npix, gather2 ? grad_d2 : nullptr, +1.0f};
  const LrcGather j1{d2, w, w + 3 * npix, gather3 ? grad_d3 : nullptr, -1.0f};
  lrcb_gather_kernel<<<grid, 256, 0, s>>>(j0, j1, H, W, map_bs, npix);
  return sa::check_launch("sa_softlrc_backward/gather");
}

extern "C" int sa_weighted_lsq_backward(const float *mde, const float *disp, const float *conf, int B, int n_per_b,
                                        const float *scale, const float *shift, const double *rec,
                                        const float *g_scale, const float *g_shift, float *grad_mde,
                                        float *grad_disp, float *grad_conf, void *stream) {
  SA_REQUIRE(mde && disp && conf && scale && shift && rec, "sa_weighted_lsq_backward: null pointer");
  SA_REQUIRE(g_scale || g_shift, "sa_weighted_lsq_backward: null pointer (both upstream gradients)");
  SA_REQUIRE(grad_mde || grad_disp || grad_conf, "sa_weighted_lsq_backward: null pointer (all three outputs)");
  SA_REQUIRE(B > 0 && B <= 65535 && n_per_b > 0, "sa_weighted_lsq_backward: empty input or B > 65535");
  SA_REQUIRE((reinterpret_cast<uintptr_t>(rec) & 7) == 0, "sa_weighted_lsq_backward: record not 8-byte aligned");
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_LSQ, s);
  const dim3 grid((unsigned)(((long)n_per_b + 255) / 256), (unsigned)B);
  lsqb_kernel<<<grid, 256, 0, s>>>(mde, disp, conf, n_per_b, scale, shift, rec, g_scale, g_shift, grad_mde, grad_disp,
                                   grad_conf);
  return sa::check_launch("sa_weighted_lsq_backward");
}

// Backward of the two remaining custom ops on the reference's fine-tuning gradient path:
// soft-argmin disparity / entropy confidence (softargmin.hip; utils.py:112-170) and convex
// up-sampling (upsample.hip; utils.py:97-110).
//
// Both are fp32 (data and per-element arithmetic; the per-line statistics E / S and the flow
// gradient's accumulator are fp64, see below) and deterministic: no floating-point atomics, one fixed
// summation order per output element.  The softmaxes are recomputed from the inputs with the line maximum subtracted, as the
// forwards do (e = exp(x - max), p = e * (1 / sum e)); nothing volume-sized is kept between forward
// and backward.
//
// Soft-argmin.  A volume has one axis of stride 1 (X, length nX) and one strided axis (Y, stride
// sy, length nY): X = k in the reference layout (sk == 1), X = j in the native one (sj == 1).  Two
// kernels per call, both volumes in one launch (blockIdx.y):
//   sab_ystats_kernel — the softmax over Y of every strided line (b, h, x): max, 1 / sum e and the
//     p-weighted sum (E or S, fp64) into the workspace, 16 bytes per line.  A lane per line, consecutive
//     lanes on consecutive x (every load a coalesced row segment), the block's 4 waves split Y.
//   sab_grad_kernel — a wave per contiguous line (b, h, y): the softmax over X of its own line
//     (max, sum, E or S by wave reductions), then the line's gradient from both sides' terms,
//     written once.
// Lines of up to 256 elements (the model's 1/4-resolution widths) are held in registers between the
// passes and their exponentials formed once; longer ones are re-read per pass (L1 / L2 hits).
// Per volume: two reads (statistics pass, gradient pass) and one write.
//
// Convex up-sampling.  cub_mask_kernel: one thread per low-res pixel and sub-pixel row a, as the
// forward's convex_up_px_kernel (a wave reads 64 consecutive floats of each mask plane and writes
// 64 consecutive floats of each gradient plane).  cub_flow_kernel: one thread per low-res pixel
// gathers its 9 neighbours' softmax weights (t, then a, then b, ascending; the neighbours' logits
// are re-read through L2, the exponentials formed again).
#include <cmath>
#include <cstdint>

#include "sa_common.h"
#include "softmax9.h"

namespace {

// ------------------------------------------------------------------------------- soft-argmin
struct SBGeo {
  int H, nX, nY;
  long sb, sh, sy;
};

// one volume: gX / gY are the upstream gradients of the outputs that reduce over X ([B,H,nY]) and
// over Y ([B,H,nX]); null: that output was not used.  cX / cY: -1 (left) / +1 (right) for the
// disparity volume, 1 / log2(reduction length) for the confidence volume.
struct SBJob {
  const float *vol;
  float *grad;
  const float *gX, *gY;
  float cX, cY;
  int mode;    // 0: disparity (index-weighted), 1: confidence (entropy)
  float *ws;   // Y-side statistics per strided line: max and 1 / sum e (floats), then E or S (doubles)
};

// E and S are accumulated and kept in fp64: where a softmax is peaked (p -> 1 at k near E) the
// gradient g p (k - E) is a small difference times a large p, and an fp32 E (a sum of terms up to W,
// then rounded to an ulp of E) shows in it at several times the error of torch's own fp32 autograd.
// They are also divided by the fp64 sum of the rounded p (1 + a few 2^-24: the rounding of 1 / sum e
// moves every p of a line by one common factor, and E with it, by up to 2^-24 E).
// One statistic per line; the per-element arithmetic is fp32.
__device__ __forceinline__ double wave_sum_f64(double v) {
  v = sa::wave_sum_dpp_lane63(v);
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), 63);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// d/dp of p log2(p + 1e-6)
__device__ __forceinline__ float ent_slope(float p) {
  const float pe = p + 1e-6f;
  return log2f(pe) + p / (pe * 0.69314718055994531f);
}

// the value a side's statistic averages and its gradient centres: the index along the reduction axis
// (disparity) or d/dp of p log2(p + 1e-6) (confidence)
__device__ __forceinline__ float stat_val(int mode, int idx, float p) { return mode == 0 ? (float)idx : ent_slope(p); }
// one side's term of the gradient: cg = coefficient x upstream gradient, T the line's fp64 statistic
__device__ __forceinline__ float grad_term(float cg, float p, float val, double T) {
  return cg * p * (float)((double)val - T);
}

// REG: a wave's segment of the line (ceil(nY / 4) <= 64 elements, nY <= 256) is loaded once and held
// in registers, its exponentials formed once; otherwise the segment is re-read per pass.  One body:
// the same operations in the same order either way, so the same bits.
template <bool REG>
__global__ __launch_bounds__(256) void sab_ystats_kernel(SBJob j0, SBJob j1, SBGeo g, long nlines) {
  __shared__ float red[2][4][64];
  __shared__ double redd[2][4][64];
  const SBJob J = blockIdx.y ? j1 : j0;
  if (!J.vol || !J.gY) return;   // block-uniform
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long line = (long)blockIdx.x * 64 + lane;
  const bool valid = line < nlines;
  const long bh = valid ? line / g.nX : 0;
  const int x = valid ? (int)(line % g.nX) : 0;
  const long b = bh / g.H, h = bh % g.H;
  const int per = (g.nY + 3) >> 2, y0 = w * per;
  const int cnt = valid ? max(0, min(per, g.nY - y0)) : 0;
  const float *src = J.vol + b * g.sb + h * g.sh + x + (long)y0 * g.sy;
  const int lim = REG ? 64 : cnt;   // REG: a compile-time bound (the loops unroll), elements past cnt masked
  float v[64];                      // (REG only)
  float m = -INFINITY;
#pragma unroll REG ? 64 : 4
  for (int i = 0; i < lim; ++i) {
    const float xi = i < cnt ? src[(long)i * g.sy] : -INFINITY;
    if constexpr (REG) v[i] = xi;
    m = fmaxf(m, xi);
  }
  red[0][w][lane] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0][0][lane], red[0][1][lane]), fmaxf(red[0][2][lane], red[0][3][lane]));
  // e_i: formed once and kept (REG) or formed again per pass
  auto expo = [&](int i) __attribute__((always_inline)) {
    if constexpr (REG) return i < cnt ? expf(v[i] - m) : 0.f;
    else return expf(src[(long)i * g.sy] - m);
  };
  float s = 0.f;
#pragma unroll REG ? 64 : 4
  for (int i = 0; i < lim; ++i) {
    const float e = expo(i);
    if constexpr (REG) v[i] = e;
    s += e;
  }
  red[1][w][lane] = s;
  __syncthreads();
  const float inv = 1.0f / ((red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]));
  double acc = 0.0, pd = 0.0;
#pragma unroll REG ? 64 : 4
  for (int i = 0; i < lim; ++i) {
    float e;
    if constexpr (REG) e = v[i];
    else e = expo(i);
    const float p = e * inv;
    if (i < cnt) {
      acc += (double)p * (double)stat_val(J.mode, y0 + i, p);
      pd += (double)p;
    }
  }
  redd[0][w][lane] = acc;
  redd[1][w][lane] = pd;
  __syncthreads();
  if (w == 0 && valid) {
    J.ws[line] = m;
    J.ws[nlines + line] = inv;
    reinterpret_cast<double *>(J.ws + 2 * nlines)[line] =
        ((redd[0][0][lane] + redd[0][1][lane]) + (redd[0][2][lane] + redd[0][3][lane])) /
        ((redd[1][0][lane] + redd[1][1][lane]) + (redd[1][2][lane] + redd[1][3][lane]));
  }
}

// One contiguous line by one wave: element lane + 64 c.  REG (n <= 256): the line's values, its
// probabilities and their stat_val stay in registers between the passes; otherwise each pass
// re-reads the line (L1 / L2 hits) and forms the exponentials again.  One body, the same bits.
template <bool REG>
__device__ __forceinline__ void grad_line(const SBJob &J, const float *__restrict__ v, float *__restrict__ out,
                                          const int n, const int y, const long line, const long bh,
                                          const long nstat, const int lane) {
  const int nc = REG ? 4 : (n + 63) >> 6;
  float xv[4], pv[4], val[4];   // (REG only)
  float m = 0.f, inv = 0.f, gl = 0.f;
  double T = 0.0;
  if constexpr (REG) {
#pragma unroll
    for (int c = 0; c < 4; ++c) xv[c] = lane + 64 * c < n ? v[lane + 64 * c] : -INFINITY;
  }
  auto value = [&](int c) __attribute__((always_inline)) {
    if constexpr (REG) return xv[c];
    else return v[lane + 64 * c];   // (called for lane + 64 c < n only)
  };
  if (J.gX) {
    m = -INFINITY;
#pragma unroll REG ? 4 : 1
    for (int c = 0; c < nc; ++c)
      if (lane + 64 * c < n) m = fmaxf(m, value(c));
    m = sa::wave_max_dpp(m);
    float s = 0.f;
#pragma unroll REG ? 4 : 1
    for (int c = 0; c < nc; ++c)
      if (lane + 64 * c < n) {
        const float e = expf(value(c) - m);
        if constexpr (REG) pv[c] = e;
        s += e;
      }
    inv = 1.0f / sa::wave_sum_dpp(s);
    double acc = 0.0, pd = 0.0;
#pragma unroll REG ? 4 : 1
    for (int c = 0; c < nc; ++c) {
      const int i = lane + 64 * c;
      if (i < n) {
        float e;
        if constexpr (REG) e = pv[c];
        else e = expf(value(c) - m);
        const float p = e * inv, a = stat_val(J.mode, i, p);
        if constexpr (REG) pv[c] = p, val[c] = a;
        acc += (double)p * (double)a;
        pd += (double)p;
      }
    }
    T = wave_sum_f64(acc) / wave_sum_f64(pd);
    gl = J.cX * J.gX[line];
  }
  const float *__restrict__ wm = nullptr, *__restrict__ wi = nullptr, *__restrict__ gy = nullptr;
  const double *__restrict__ wt = nullptr;
  if (J.gY) {   // the strided side's statistics of this (b, h): indexed like the line
    wm = J.ws + bh * n;
    wi = wm + nstat;
    wt = reinterpret_cast<const double *>(J.ws + 2 * nstat) + bh * n;
    gy = J.gY + bh * n;
  }
#pragma unroll REG ? 4 : 1
  for (int c = 0; c < nc; ++c) {
    const int i = lane + 64 * c;
    if (i >= n) continue;
    const float x = value(c);
    float r = 0.f;
    if (J.gX) {
      float p, a;
      if constexpr (REG) p = pv[c], a = val[c];
      else p = expf(x - m) * inv, a = stat_val(J.mode, i, p);
      r = grad_term(gl, p, a, T);
    }
    if (J.gY) {
      const float q = expf(x - wm[i]) * wi[i];
      r += grad_term(J.cY * gy[i], q, stat_val(J.mode, y, q), wt[i]);
    }
    out[i] = r;
  }
}

__global__ __launch_bounds__(256) void sab_grad_kernel(SBJob j0, SBJob j1, SBGeo g, long nlines, long nstat) {
  const SBJob J = blockIdx.y ? j1 : j0;
  if (!J.vol) return;
  const long line = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (line >= nlines) return;   // wave-uniform
  const int lane = threadIdx.x & 63;
  const long bh = line / g.nY;
  const int y = (int)(line % g.nY);
  const long b = bh / g.H, h = bh % g.H;
  const long base = b * g.sb + h * g.sh + (long)y * g.sy;
  if (g.nX <= 256)   // wave-uniform
    grad_line<true>(J, J.vol + base, J.grad + base, g.nX, y, line, bh, nstat, lane);
  else
    grad_line<false>(J, J.vol + base, J.grad + base, g.nX, y, line, bh, nstat, lane);
}

// ------------------------------------------------------------------------- convex up-sampling
// thread = (b, a, h, w), w fastest; F: the factor at compile time (0: f_rt)
template <int F>
__global__ __launch_bounds__(256) void cub_mask_kernel(const float *__restrict__ flow, const float *__restrict__ mask,
                                                       long mask_bs, const float *__restrict__ gout, int H, int W,
                                                       int f_rt, float scale, long n, float *__restrict__ gmask) {
  const int f = F ? F : f_rt;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long hw = (long)H * W;
  const int w = (int)(i % W);
  const long q = i / W;
  const int h = (int)(q % H);
  const int a = (int)((q / H) % f);
  const long b = q / ((long)H * f);
  const float *fl = flow + b * hw;
  float u[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {   // clamped loads, then the zero padding as a select
    const int yy = h + k / 3 - 1, xx = w + k % 3 - 1;
    const float t = fl[(long)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1)];
    u[k] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? scale * t : 0.0f;
  }
  const long kstride = (long)f * f * hw;
  const long off = (long)(a * f) * hw + (long)h * W + w;
  const float *m = mask + b * mask_bs + off;
  float *gm = gmask + b * 9 * kstride + off;
  const float *go = gout + b * hw * f * f + (long)(h * f + a) * ((long)W * f) + (long)w * f;
#pragma unroll
  for (int c = 0; c < (F ? F : 8); ++c) {
    if (c >= f) break;
    float s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] = m[k * kstride + (long)c * hw];
    sa::softmax9(s);
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) dot += s[k] * u[k];
    const float gv = go[c];
#pragma unroll
    for (int k = 0; k < 9; ++k) gm[k * kstride + (long)c * hw] = s[k] * (u[k] - dot) * gv;
  }
}

// thread = (b, y, x), x fastest; F: the factor at compile time (4: the (a, b) loops unroll, so a
// neighbour's 144 logits are all in flight together), 0: f_rt
template <int F>
__global__ __launch_bounds__(256) void cub_flow_kernel(const float *__restrict__ mask, long mask_bs,
                                                       const float *__restrict__ gout, int H, int W, int f_rt,
                                                       float scale, long n, float *__restrict__ gflow) {
  const int f = F ? F : f_rt;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long hw = (long)H * W;
  const int x = (int)(i % W);
  const int y = (int)((i / W) % H);
  const long b = i / hw;
  const long kstride = (long)f * f * hw;
  const long Wo = (long)W * f;
  const float *mb = mask + b * mask_bs;
  const float *gb = gout + b * hw * f * f;
  // (an fp64 accumulator: the 9 f f terms, each an exact product of two floats, are summed without
  // rounding to fp32 in between; a running fp32 sum of the 144 - 576 terms is at 4.5x the error of
  // torch's own fp32 autograd, which is one ulp of the result here)
  double acc = 0.0;
  for (int t = 0; t < 9; ++t) {
    const int yy = y - (t / 3 - 1), xx = x - (t % 3 - 1);   // the pixel whose tap t is (y, x)
    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
    const float *m = mb + (long)yy * W + xx;
    const float *go = gb + (long)yy * f * Wo + (long)xx * f;
#pragma unroll F ? F : 1
    for (int a = 0; a < f; ++a)
#pragma unroll F ? F : 1
      for (int c = 0; c < f; ++c) {
        float s[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] = m[k * kstride + (long)(a * f + c) * hw];
        sa::softmax9(s);
        float st = s[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) st = k == t ? s[k] : st;   // (no run-time register index)
        acc += (double)st * (double)go[a * Wo + c];
      }
  }
  gflow[i] = scale * (float)acc;
}

}  // namespace

extern "C" long sa_softargmin_conf_backward_ws_size(int B, int H, int W1, int W2) {
  if (B <= 0 || H <= 0 || W1 <= 1 || W2 <= 1) return -1;
  return 2L * 4L * B * H * (W1 > W2 ? W1 : W2) * (long)sizeof(float);
}

extern "C" int sa_softargmin_conf_backward(const float *vol_disp, const float *vol_conf, int B, int H, int W1, int W2,
                                           long sb, long sh, long sj, long sk, const float *g_dL, const float *g_dR,
                                           const float *g_cL, const float *g_cR, float *grad_vol_disp,
                                           float *grad_vol_conf, void *ws, void *stream) {
  const bool use_d = g_dL || g_dR, use_c = g_cL || g_cR;
  SA_REQUIRE(use_d || use_c, "sa_softargmin_conf_backward: null pointer (all four upstream gradients)");
  SA_REQUIRE(!use_d || (vol_disp && grad_vol_disp), "sa_softargmin_conf_backward: null pointer (vol_disp / grad_vol_disp)");
  SA_REQUIRE(!use_c || (vol_conf && grad_vol_conf), "sa_softargmin_conf_backward: null pointer (vol_conf / grad_vol_conf)");
  SA_REQUIRE(B > 0 && H > 0 && W1 > 1 && W2 > 1, "sa_softargmin_conf_backward: bad shape (B, H > 0; W1, W2 > 1)");
  SA_REQUIRE(sj == 1 || sk == 1, "sa_softargmin_conf_backward: one of sj/sk must be 1");
  SA_REQUIRE(sb >= 0 && sh >= 0 && sj >= 1 && sk >= 1, "sa_softargmin_conf_backward: strides must be positive");
  const bool ref = sk == 1;   // X = k: the left side reduces along the contiguous axis
  // the workspace holds the strided side's statistics: read and written only when that side has a gradient
  const bool need_ws = ref ? (g_dR || g_cR) : (g_dL || g_cL);
  SA_REQUIRE(!need_ws || ws,
             "sa_softargmin_conf_backward: null pointer (workspace of sa_softargmin_conf_backward_ws_size bytes)");
  SA_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "sa_softargmin_conf_backward: workspace must be 8-byte aligned");
  SBGeo g{H, ref ? W2 : W1, ref ? W1 : W2, sb, sh, ref ? sj : sk};
  const long nlY = (long)B * H * g.nY;   // contiguous lines (one per y)
  const long nlX = (long)B * H * g.nX;   // strided lines (one per x)
  SA_REQUIRE((nlY + 3) / 4 < (1L << 31) && (nlX + 63) / 64 < (1L << 31), "sa_softargmin_conf_backward: grid too large");
  float *w = static_cast<float *>(ws);
  const float rl1 = (float)(1.0 / std::log2((double)W1)), rl2 = (float)(1.0 / std::log2((double)W2));
  // left outputs reduce over k (length W2), right outputs over j (length W1)
  SBJob jd{use_d ? vol_disp : nullptr, grad_vol_disp, ref ? g_dL : g_dR, ref ? g_dR : g_dL,
           ref ? -1.0f : 1.0f, ref ? 1.0f : -1.0f, 0, w};   // (ws null: no gY, never used)
  SBJob jc{use_c ? vol_conf : nullptr, grad_vol_conf, ref ? g_cL : g_cR, ref ? g_cR : g_cL,
           ref ? rl2 : rl1, ref ? rl1 : rl2, 1, w ? w + 4 * nlX : nullptr};
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  if (need_ws) {
    const dim3 grid((unsigned)((nlX + 63) / 64), 2u);
    if (g.nY <= 256)
      sab_ystats_kernel<true><<<grid, 256, 0, s>>>(jd, jc, g, nlX);
    else
      sab_ystats_kernel<false><<<grid, 256, 0, s>>>(jd, jc, g, nlX);
    const int rc = sa::check_launch("sa_softargmin_conf_backward");
    if (rc) return rc;
  }
  sab_grad_kernel<<<dim3((unsigned)((nlY + 3) / 4), 2u), 256, 0, s>>>(jd, jc, g, nlY, nlX);
  return sa::check_launch("sa_softargmin_conf_backward");
}

extern "C" int sa_convex_upsample_backward(const float *flow, const float *mask, long mask_bs, const float *grad_out,
                                           int B, int H, int W, int factor, float scale, float *grad_flow,
                                           float *grad_mask, void *stream) {
  SA_REQUIRE(mask && grad_out, "sa_convex_upsample_backward: null pointer (mask / grad_out)");
  SA_REQUIRE(grad_flow || grad_mask, "sa_convex_upsample_backward: null pointer (grad_flow and grad_mask)");
  SA_REQUIRE(!grad_mask || flow, "sa_convex_upsample_backward: null pointer (flow, read by grad_mask)");
  SA_REQUIRE(B > 0 && H > 0 && W > 0, "sa_convex_upsample_backward: empty shape");
  SA_REQUIRE(factor >= 1 && factor <= 8, "sa_convex_upsample_backward: factor must be 1..8");
  SA_REQUIRE(mask_bs >= 9L * factor * factor * H * W, "sa_convex_upsample_backward: mask batch stride too small");
  const long np = (long)B * H * W;
  SA_REQUIRE((np * factor + 255) / 256 < (1L << 31), "sa_convex_upsample_backward: grid too large");
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  if (grad_mask) {
    const long n = np * factor;
    const unsigned nb = (unsigned)((n + 255) / 256);
    if (factor == 4)
      cub_mask_kernel<4><<<nb, 256, 0, s>>>(flow, mask, mask_bs, grad_out, H, W, 4, scale, n, grad_mask);
    else
      cub_mask_kernel<0><<<nb, 256, 0, s>>>(flow, mask, mask_bs, grad_out, H, W, factor, scale, n, grad_mask);
    const int rc = sa::check_launch("sa_convex_upsample_backward");
    if (rc) return rc;
  }
  if (grad_flow) {
    const unsigned nb = (unsigned)((np + 255) / 256);
    if (factor == 4)
      cub_flow_kernel<4><<<nb, 256, 0, s>>>(mask, mask_bs, grad_out, H, W, 4, scale, np, grad_flow);
    else
      cub_flow_kernel<0><<<nb, 256, 0, s>>>(mask, mask_bs, grad_out, H, W, factor, scale, np, grad_flow);
  }
  return sa::check_launch("sa_convex_upsample_backward");
}

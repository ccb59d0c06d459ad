// Mono-scale alignment: softLRC, weighted LSQ with exact quantile band, mirror
// detector and initial coordinates.
//
// Reference: softlrc + disp_warping (utils.py:172-198), fuzzy_and (240-241),
// weighted_lsq (345-384), scaled mono maps (stereoanywhere.py:191-199),
// handcrafted_mirror_detector (utils.py:255-269), coords init (stereoanywhere.py:261-262).
//
// The reference's weighted_lsq runs torch.quantile + boolean indexing +
// torch.linalg.lstsq per sample: host syncs and a CPU-side LAPACK call on GPU.  Here
// one workgroup per sample finds the four order statistics the two linear quantiles
// need by an 8-bit-per-pass radix select on the float bits (relu'd values are
// non-negative, so their bit patterns order like the values), then accumulates the
// 2x2 weighted normal equations in float64 and solves them — no host round trip.
#include <cmath>
#include <cstdint>

#include "lrc_sample.h"
#include "lsq_select.h"
#include "sa_common.h"

namespace {

// ------------------------------------------------------------------ softLRC
using sa::softplus_ref;

// grid_sample(bilinear, zeros, align_corners=True) of one [H,W] plane at the grid
// point (gx, gy) already normalised to [-1, 1] (the taps: lrc_sample.h).
__device__ __forceinline__ float sample_zero_ac(const float *__restrict__ img, int H, int W, float gx,
                                                float gy) {
  const sa::LrcTaps t = sa::lrc_taps(H, W, gx, gy);
  const int xi = t.xi, yi = t.yi;
  // (the test of sa::lrc_inside, spelled out: through the call this kernel compiles to other code)
  auto at = [&](int y, int x) {
    return (x >= 0 && x <= W - 1 && y >= 0 && y <= H - 1) ? img[(long)y * W + x] : 0.0f;
  };
  return at(yi, xi) * t.nw + at(yi, xi + 1) * t.ne + at(yi + 1, xi) * t.sw + at(yi + 1, xi + 1) * t.se;
}

// softlrc of pixel (y, x): compare d_self with d_other warped by relu(d_src)
// sign = -1: left map (sample at x - relu(d2)), +1: right map (x + relu(d3)).
__device__ __forceinline__ float softlrc_px(const float *__restrict__ dself, const float *__restrict__ dother,
                                            int H, int W, int y, int x, float sign, float th,
                                            float div) {
  const float dsrc = fmaxf(dself[(long)y * W + x], 0.0f);
  float gx, gy;
  sa::lrc_grid(H, W, y, x, dsrc, sign, gx, gy);
  const float warped = sample_zero_ac(dother, H, W, gx, gy);
  const float d = dself[(long)y * W + x];
  return softplus_ref(-fabsf(d - warped) + th) / div;
}

__global__ __launch_bounds__(256) void softlrc_kernel(const float *__restrict__ d2, const float *__restrict__ d3,
                                                      const float *__restrict__ c2, const float *__restrict__ c3,
                                                      int H, int W, long bs, float th, float div, long npix,
                                                      float *__restrict__ s2, float *__restrict__ s3) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const long hw = (long)H * W;
  const long b = p / hw, r = p % hw;
  const int y = (int)(r / W), x = (int)(r % W);
  const float *a = d2 + b * bs, *c = d3 + b * bs;
  // softlrc_disp2 uses warped_disp3 = disp_warping(relu(disp2), disp3, right_disp=False)
  float v2 = softlrc_px(a, c, H, W, y, x, -1.0f, th, div);
  float v3 = softlrc_px(c, a, H, W, y, x, +1.0f, th, div);
  if (c2) v2 = c2[b * bs + r] * v2;
  if (c3) v3 = c3[b * bs + r] * v3;
  s2[b * bs + r] = v2;
  s3[b * bs + r] = v3;
}

// ------------------------------------------------------------------ weighted LSQ
// (the one-launch kernel lsq1_kernel and the selection helpers: lsq_select.h)

// ---------------------------------------------------- weighted LSQ, grid-wide variant
// The same radix select and normal equations spread over LSQ_NB(n) blocks per sample:
// one launch per 8-bit digit, each block histograms its slice in LDS and adds the
// non-zero bins to the sample's global histogram; the block that finishes last (an
// arrival counter) selects the digit for the next launch and clears the histogram.  The
// final launch forms per-block float64 partials that the last block sums in block order
// (deterministic) before solving.  Workspace per sample, zeroed before the first launch:
//   LsqState (64 B) | hist[4][256] u32 | part[nb][5] f64.
constexpr int LSQ_BT = 256, LSQ_EPT = 8, LSQ_CH = LSQ_BT * LSQ_EPT;

struct LsqState {
  unsigned prefix[4], remain[4], count, pad[7];
};

inline int lsq_nb(int n) { return (n + LSQ_CH - 1) / LSQ_CH; }
inline long lsq_ws_stride(int n) { return ((64 + 4096 + (long)lsq_nb(n) * 40) + 255) / 256 * 256; }

__device__ __forceinline__ unsigned ld_agent(const unsigned *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void lsq_initial_ranks(int n, float q_lo, float q_hi, int r, unsigned &rem) {
  const float rk = (r < 2 ? q_lo : q_hi) * (float)(n - 1);
  rem = (unsigned)((r & 1) ? ceilf(rk) : truncf(rk));
}

__global__ __launch_bounds__(LSQ_BT) void lsq_hist_kernel(const float *__restrict__ disp, int n, int nb, float q_lo,
                                                          float q_hi, int pass, char *__restrict__ ws, long wss) {
  __shared__ unsigned hist[4][256];
  __shared__ unsigned s_pre[4], s_rem[4];
  __shared__ int s_last;
  const int b = blockIdx.x / nb, j = blockIdx.x % nb;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  LsqState *st = reinterpret_cast<LsqState *>(ws + b * wss);
  unsigned *gh = reinterpret_cast<unsigned *>(ws + b * wss + 64);
  if (t < 4) {
    if (pass == 0) {
      lsq_initial_ranks(n, q_lo, q_hi, t, s_rem[t]);
      s_pre[t] = 0u;
    } else {
      s_pre[t] = st->prefix[t];
      s_rem[t] = st->remain[t];
    }
  }
  for (int i = t; i < 4 * 256; i += LSQ_BT) (&hist[0][0])[i] = 0u;
  __syncthreads();
  const int shift_ = 24 - 8 * pass;
  unsigned pre[4];
  int src[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    pre[r] = s_pre[r];
    src[r] = r;
    for (int q = r - 1; q >= 0; --q)
      if (pre[q] == pre[r]) src[r] = q;
  }
  const float *dd = disp + (long)b * n + (long)j * LSQ_CH;
  const int cnt = min(LSQ_CH, n - j * LSQ_CH);
  unsigned keys[LSQ_EPT];
#pragma unroll
  for (int i = 0; i < LSQ_EPT; ++i) keys[i] = t + i * LSQ_BT < cnt ? key_of(dd[t + i * LSQ_BT]) : 0u;
#pragma unroll
  for (int i = 0; i < LSQ_EPT; ++i) {
    const bool valid = t + i * LSQ_BT < cnt;
    const unsigned bin = (keys[i] >> shift_) & 255u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (src[r] != r) continue;
      const bool match = valid && (pass == 0 || ((keys[i] ^ pre[r]) >> (shift_ + 8)) == 0u);
      hist_add(hist[r], bin, match);
    }
  }
  __syncthreads();
  for (int i = t; i < 4 * 256; i += LSQ_BT) {
    const unsigned c = (&hist[0][0])[i];
    if (c && src[i >> 8] == (i >> 8)) atomicAdd(&gh[i], c);
  }
  __threadfence();
  __syncthreads();
  if (t == 0) s_last = atomicAdd(&st->count, 1u) == (unsigned)(nb - 1);
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  if (wv < 4) {
    const unsigned *hr = gh + 256 * pick4(src, wv);
    const unsigned rem = s_rem[wv];
    const unsigned c0 = ld_agent(hr + 4 * lane), c1 = ld_agent(hr + 4 * lane + 1);
    const unsigned c2 = ld_agent(hr + 4 * lane + 2), c3 = ld_agent(hr + 4 * lane + 3);
    unsigned inc = c0 + c1 + c2 + c3;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    const unsigned long long past = __ballot(inc > rem);
    const int L = past ? __ffsll((long long)past) - 1 : 63;
    if (lane == L) {
      unsigned acc = inc - (c0 + c1 + c2 + c3), sel = 4u * L + 3u;
      const unsigned cs[4] = {c0, c1, c2, c3};
      for (int k = 0; k < 4; ++k) {
        if (acc + cs[k] > rem) {
          sel = 4u * L + k;
          break;
        }
        acc += cs[k];
      }
      st->remain[wv] = rem - acc;
      st->prefix[wv] = pick4(pre, wv) | (sel << shift_);
    }
  }
  __syncthreads();
  for (int i = t; i < 4 * 256; i += LSQ_BT) gh[i] = 0u;
  if (t == 0) st->count = 0u;
}

__global__ __launch_bounds__(LSQ_BT) void lsq_solve_kernel(const float *__restrict__ mde, const float *__restrict__ disp,
                                                           const float *__restrict__ conf, int n, int nb, float q_lo,
                                                           float q_hi, char *__restrict__ ws, long wss,
                                                           float *__restrict__ scale, float *__restrict__ shift) {
  __shared__ double red[5][LSQ_BT / 64];
  __shared__ int s_last;
  const int b = blockIdx.x / nb, j = blockIdx.x % nb;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  LsqState *st = reinterpret_cast<LsqState *>(ws + b * wss);
  double *part = reinterpret_cast<double *>(ws + b * wss + 64 + 4096);
  const float r_lo = q_lo * (float)(n - 1), r_hi = q_hi * (float)(n - 1);
  const float qlo = lerp_ref(__uint_as_float(st->prefix[0]), __uint_as_float(st->prefix[1]), r_lo - truncf(r_lo));
  const float qhi = lerp_ref(__uint_as_float(st->prefix[2]), __uint_as_float(st->prefix[3]), r_hi - truncf(r_hi));
  const long off = (long)b * n + (long)j * LSQ_CH;
  const int cnt = min(LSQ_CH, n - j * LSQ_CH);
  double acc[5] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < LSQ_EPT; ++i) {
    const int e = t + i * LSQ_BT;
    if (e >= cnt) continue;
    const float d = __uint_as_float(key_of(disp[off + e]));
    if (qlo <= d && d <= qhi) {
      const float m = fabsf(mde[off + e]);
      const float c = fabsf(conf[off + e]) * 0.9f + 0.1f;
      const float w = sqrtf(c);
      const float a1 = m * w, y = fabsf(d) * w;
      acc[0] += (double)a1 * a1;
      acc[1] += (double)a1 * w;
      acc[2] += (double)w * w;
      acc[3] += (double)a1 * y;
      acc[4] += (double)w * y;
    }
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    double v = acc[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) red[q][wv] = v;
  }
  __syncthreads();
  if (t < 5) part[j * 5 + t] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
  __threadfence();
  __syncthreads();
  if (t == 0) s_last = atomicAdd(&st->count, 1u) == (unsigned)(nb - 1);
  __syncthreads();
  if (!s_last || t != 0) return;
  __threadfence();
  double s[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < nb; ++k)
    for (int q = 0; q < 5; ++q)
      s[q] += __hip_atomic_load(part + k * 5 + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  st->count = 0u;
  const double s11 = s[0], s12 = s[1], s22 = s[2], t1 = s[3], t2 = s[4];
  const double det = s11 * s22 - s12 * s12;
  double sc, sh;
  if (s22 > 0 && fabs(det) > 1e-12 * s11 * s22) {
    sc = (s22 * t1 - s12 * t2) / det;
    sh = (s11 * t2 - s12 * t1) / det;
  } else if (s22 > 0) {
    const double m0 = s12 / s22, c0 = t2 / s22;
    sc = c0 * m0 / (m0 * m0 + 1.0);
    sh = c0 / (m0 * m0 + 1.0);
  } else {
    sc = 0.0;
    sh = 0.0;
  }
  scale[b] = (float)sc;
  shift[b] = (float)sh;
}

// ------------------------------------------------------------------ scaled mono + mirror
__global__ __launch_bounds__(256) void scale_maps_kernel(const float *__restrict__ m2, const float *__restrict__ m3,
                                                         const float *__restrict__ scale,
                                                         const float *__restrict__ shift, long hw, long in_bs,
                                                         long npix, float *__restrict__ sm2,
                                                         float *__restrict__ sm3) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const long b = p / hw, r = p % hw;
  const float s = scale[b], t = shift[b];
  sm2[p] = s * m2[b * in_bs + r] + t;
  sm3[p] = s * m3[b * in_bs + r] + t;
}

__global__ __launch_bounds__(256) void mirror_kernel(const float *__restrict__ sm2, const float *__restrict__ sm3,
                                                     const float *__restrict__ dL, const float *__restrict__ confl,
                                                     int H, int W, long in_bs, float th, float div,
                                                     float conf_th, long npix, float *__restrict__ mirror,
                                                     float *__restrict__ coords_x) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const long hw = (long)H * W;
  const long b = p / hw, r = p % hw;
  const int y = (int)(r / W), x = (int)(r % W);
  const float lrc = softlrc_px(sm2 + b * hw, sm3 + b * hw, H, W, y, x, -1.0f, th, div);
  const float sc = confl[b * in_bs + r], md = sm2[p], sd = dL[b * in_bs + r];
  const float both = sc * lrc;
  const float near_ = sa::sigmoidf_ref(20.0f * (md - sd));
  const float a = both * near_;
  const float bb = (1.0f - sc) * lrc;
  const float better = a + bb - a * bb;
  mirror[p] = sa::sigmoidf_ref(20.0f * (better - conf_th));
  coords_x[p] = (float)x - md;
}

}  // namespace

extern "C" int sa_softlrc(const float *d2, const float *d3, const float *conf2, const float *conf3, int B,
                          int H, int W, long map_bs, float lrc_th, float *s2, float *s3, void *stream) {
  SA_REQUIRE(d2 && d3 && s2 && s3, "sa_softlrc: null pointer");
  SA_REQUIRE(B > 0 && H > 0 && W > 0, "sa_softlrc: empty shape");
  SA_REQUIRE(map_bs >= (long)H * W, "sa_softlrc: map_bs too small");
  const long npix = (long)B * H * W;
  const float div = (float)std::log(1.0 + std::exp((double)lrc_th));
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  softlrc_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, s>>>(d2, d3, conf2, conf3, H, W, map_bs, lrc_th,
                                                                div, npix, s2, s3);
  return sa::check_launch("sa_softlrc");
}

extern "C" int sa_weighted_lsq(const float *mde, const float *disp, const float *conf, int B, int n_per_b,
                               float q_lo, float q_hi, float *scale, float *shift, void *stream) {
  SA_REQUIRE(mde && disp && conf && scale && shift, "sa_weighted_lsq: null pointer");
  SA_REQUIRE(B > 0 && n_per_b > 0, "sa_weighted_lsq: empty input");
  SA_REQUIRE(q_lo >= 0.f && q_lo <= q_hi && q_hi <= 1.f, "sa_weighted_lsq: quantiles out of order");
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_LSQ, s);
  lsq1_kernel<false><<<B, LSQ_THREADS, 0, s>>>(mde, disp, conf, n_per_b, q_lo, q_hi, scale, shift);
  return sa::check_launch("sa_weighted_lsq");
}

extern "C" long sa_weighted_lsq_ws_size(int B, int n_per_b) {
  if (B <= 0 || n_per_b <= 0) return -1;
  return (long)B * lsq_ws_stride(n_per_b);
}

extern "C" int sa_weighted_lsq_ws(const float *mde, const float *disp, const float *conf, int B, int n_per_b,
                                  float q_lo, float q_hi, float *scale, float *shift, void *ws, void *stream) {
  SA_REQUIRE(mde && disp && conf && scale && shift && ws, "sa_weighted_lsq_ws: null pointer");
  SA_REQUIRE(B > 0 && n_per_b > 0, "sa_weighted_lsq_ws: empty input");
  SA_REQUIRE(q_lo >= 0.f && q_lo <= q_hi && q_hi <= 1.f, "sa_weighted_lsq_ws: quantiles out of order");
  SA_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "sa_weighted_lsq_ws: workspace not 16-byte aligned");
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_LSQ, s);
  const int nb = lsq_nb(n_per_b);
  const long wss = lsq_ws_stride(n_per_b);
  char *w = static_cast<char *>(ws);
  for (int pass = 0; pass < 4; ++pass) {
    lsq_hist_kernel<<<(unsigned)(B * nb), LSQ_BT, 0, s>>>(disp, n_per_b, nb, q_lo, q_hi, pass, w, wss);
    const int rc = sa::check_launch("sa_weighted_lsq_ws/hist");
    if (rc) return rc;
  }
  lsq_solve_kernel<<<(unsigned)(B * nb), LSQ_BT, 0, s>>>(mde, disp, conf, n_per_b, nb, q_lo, q_hi, w, wss, scale,
                                                         shift);
  return sa::check_launch("sa_weighted_lsq_ws/solve");
}

extern "C" int sa_mono_scale_mirror(const float *m2, const float *m3, const float *scale, const float *shift,
                                    const float *dL, const float *conf_l, int B, int H, int W, long in_bs,
                                    float lrc_th, float conf_th, float *sm2, float *sm3, float *mirror,
                                    float *coords_x, void *stream) {
  SA_REQUIRE(m2 && m3 && scale && shift && dL && conf_l && sm2 && sm3 && mirror && coords_x,
             "sa_mono_scale_mirror: null pointer");
  SA_REQUIRE(B > 0 && H > 0 && W > 0, "sa_mono_scale_mirror: empty shape");
  SA_REQUIRE(in_bs >= (long)H * W, "sa_mono_scale_mirror: in_bs too small");
  const long npix = (long)B * H * W;
  const float div = (float)std::log(1.0 + std::exp((double)lrc_th));
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  const unsigned nb = (unsigned)((npix + 255) / 256);
  scale_maps_kernel<<<nb, 256, 0, s>>>(m2, m3, scale, shift, (long)H * W, in_bs, npix, sm2, sm3);
  int rc = sa::check_launch("sa_mono_scale_mirror/scale");
  if (rc) return rc;
  mirror_kernel<<<nb, 256, 0, s>>>(sm2, sm3, dL, conf_l, H, W, in_bs, lrc_th, div, conf_th, npix, mirror, coords_x);
  return sa::check_launch("sa_mono_scale_mirror/mirror");
}

// weighted_lsq in one launch: the radix-select helpers and lsq1_kernel (one workgroup per sample).
// A header because the kernel has two instances in two translation units: lsq.hip instantiates the
// one behind sa_weighted_lsq, lsq_stats.hip the one that also writes the backward's record
// (sa_weighted_lsq_stats).  Kept apart so that the first is compiled exactly as it was before the
// second existed: with both in one file the inliner's choices, and with them the first instance's
// code, changed.
#pragma once

#include <cmath>
#include <cstdint>

#include "sa_common.h"

namespace {

// ------------------------------------------------------------------ weighted LSQ
constexpr int LSQ_THREADS = 1024;

__device__ __forceinline__ unsigned key_of(float d) {
  d = fmaxf(d, 0.0f);  // F.relu (utils.py:352)
  if (d == 0.0f) d = 0.0f;  // -0 -> +0 so bit order == value order
  return __float_as_uint(d);
}

__device__ __forceinline__ float lerp_ref(float a, float b, float w) {
  // at::lerp CPU: |w| < 0.5 ? a + w (b - a) : b - (b - a)(1 - w)
  return fabsf(w) < 0.5f ? a + w * (b - a) : b - (b - a) * (1.0f - w);
}

__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < LSQ_THREADS / 64; ++i) t += red[i];  // fixed order: deterministic
  return t;
}

// LDS histogram add of one key per lane.  Keys of a wave often share a few bins (the
// high digits: sign and exponent; clustered values): the lanes of each of the first few
// distinct bins are counted with one atomic of their number instead of a many-way
// same-address conflict; lanes left after that add one each.
__device__ __forceinline__ void hist_add(unsigned *h, unsigned bin, bool count) {
  unsigned long long act = __ballot(count);
  const unsigned long long me = 1ull << (threadIdx.x & 63);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    if (!act) return;
    const int leader = __ffsll((long long)act) - 1;   // (wave-uniform: a v_readlane, not an LDS round trip)
    const unsigned lb = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);
    const unsigned long long same = __ballot((act & me) && bin == lb);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[lb], (unsigned)__popcll(same));
    act &= ~same;
  }
  if (act & me) atomicAdd(&h[bin], 1u);
}

// ------------------------------------------------- weighted LSQ, one launch (round 6)
// One workgroup of 1024 threads per sample, one launch for the whole batch.  The four order
// statistics (floor / ceil ranks of the two linear quantiles) come from one pass over the keys
// instead of four radix passes:
//   A. a histogram of the top 15 bits of every key (relu'd values: sign 0, so 16384 bins of
//      relative width 2^-6) in LDS; a wave per rank finds the rank's bin and the count below it
//      (per-thread sums of 8 bins, then the bins of the one segment);
//   B. the keys of the (at most 4, usually 2) selected bins are copied into an LDS
//      pool at offsets known from the histogram (the pool holds 16384 keys: 25 % of a model sample);
//      the same pass accumulates the normal equations of every key in a bin strictly between the
//      lower and the upper quantile's bins (inside the band whatever the exact quantiles);
//   C. a 9-bit and an 8-bit radix pass over each rank's bin (its pool slice) give the exact key;
//      then one more pass over the keys, in index order, adds the terms of the selected bins' keys
//      that are inside the band (the order of pool[] depends on wave timing; the sums must not).
// A sample whose selected bins hold more keys than the pool (e.g. a quarter of the pixels at
// one value) takes the four full 8-bit radix passes instead (lsq_select_radix below, the round-5
// single-block algorithm) and a separate pass for the normal equations, in the same launch.
// Every pass streams the sample's keys from memory (L2-resident after the first) in chunks of
// L1_CH keys per thread whose loads are all in flight together: one load at a time, the pass
// would wait a round trip per key.
constexpr int L1_BINS = 16384, L1_SHIFT = 17, L1_POOL = 16384, L1_SEG = 8, L1_CH = 16;
// Bin 0 holds the exact zeros alone, bin b >= 1 the positive keys whose top bits are b - 1: the
// relu'd zeros can be half of a sample (the model's synthetic-weight disparities; an edge's
// out-of-view pixels), and a quantile among them is exactly 0 without pooling or a radix pass (in
// one shared bin with the smallest positive keys they overflowed the pool: the four-pass fallback,
// 177 against ~75 us).  The largest key (NaN 0x7fc00000) maps to bin 16353 < L1_BINS.
__device__ __forceinline__ unsigned bin_of(unsigned k) { return k ? (k >> L1_SHIFT) + 1u : 0u; }

// f(key, index, valid) over this thread's keys of dd[0 .. n), in chunks of L1_CH loads in flight
template <class Fn>
__device__ __forceinline__ void lsq_stream_keys(const float *__restrict__ dd, int n, Fn f) {
  const int t = threadIdx.x;
  for (int base = 0; base < n; base += L1_CH * LSQ_THREADS) {
    unsigned k[L1_CH];
#pragma unroll
    for (int c = 0; c < L1_CH; ++c)   // (clamped, not predicated: a load under a branch waits at once)
      k[c] = key_of(dd[min(base + c * LSQ_THREADS + t, n - 1)]);
#pragma unroll
    for (int c = 0; c < L1_CH; ++c) {
      const int j = base + c * LSQ_THREADS + t;
      f(k[c], j, j < n);
    }
  }
}

// a[i] of a 4-entry register array for a wave-uniform i < 4 (no dynamic indexing: that goes to scratch)
template <class T>
__device__ __forceinline__ T pick4(const T (&a)[4], int i) {
  return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3];
}

// the first index i of cnt[0 .. 64 * PER) (LDS) whose inclusive prefix count exceeds rem, and the
// count of the entries before it; every lane of the calling wave gets both
template <int PER>
__device__ __forceinline__ void wave_find(const unsigned *cnt, unsigned rem, int &idx, unsigned &below) {
  const int lane = threadIdx.x & 63;
  unsigned c[PER], tot = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    c[k] = cnt[lane * PER + k];
    tot += c[k];
  }
  unsigned inc = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  const unsigned long long past = __ballot(inc > rem);
  const int L = past ? __ffsll((long long)past) - 1 : 63;
  unsigned acc = inc - tot;
  int sel = PER - 1;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (acc + c[k] > rem) {
      sel = k;
      break;
    }
    acc += c[k];
  }
  idx = __shfl(L * PER + sel, L);
  below = __shfl(acc, L);
}

// The round-5 single-block selection: four 8-bit radix passes over all n keys (re-read from
// memory), ranks sharing a prefix share a histogram.  hist: LDS [4][256]; pre / rem: LDS [4]
// (rem holds the ranks on entry, the keys' prefixes in pre on exit).
__device__ __forceinline__ void lsq_select_radix(const float *__restrict__ dd, int n, unsigned *hist, unsigned *prefix,
                                 unsigned *remain) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t < 4) prefix[t] = 0u;
  __syncthreads();
  for (int pass = 0; pass < 4; ++pass) {
    const int shift_ = 24 - 8 * pass;
    for (int i = t; i < 4 * 256; i += LSQ_THREADS) hist[i] = 0u;
    __syncthreads();
    unsigned pre[4];
    int src[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pre[r] = prefix[r];
      src[r] = r;
      for (int q = r - 1; q >= 0; --q)
        if (pre[q] == pre[r]) src[r] = q;
    }
    lsq_stream_keys(dd, n, [&](unsigned k, int, bool valid) {
      const unsigned bin = (k >> shift_) & 255u;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (src[r] != r) continue;
        const bool match = valid && (pass == 0 || ((k ^ pre[r]) >> (shift_ + 8)) == 0u);
        hist_add(hist + 256 * r, bin, match);
      }
    });
    __syncthreads();
    if (wv < 4) {
      int d;
      unsigned below;
      wave_find<4>(hist + 256 * pick4(src, wv), remain[wv], d, below);
      if (lane == 0) {
        remain[wv] -= below;
        prefix[wv] = pick4(pre, wv) | ((unsigned)d << shift_);
      }
    }
    __syncthreads();
  }
}

// STATS: the instance behind sa_weighted_lsq_stats (lsq_stats.hip); it also writes the sample's
// record for sa_weighted_lsq_backward (SA_LSQ_REC doubles, the layout in stereoanywhere_hip.h) through
// one more argument, double *rec.  The instance without it is sa_weighted_lsq's (lsq.hip), with the
// arguments it always had.
template <bool STATS, class... Rec>
__global__ __launch_bounds__(LSQ_THREADS) void lsq1_kernel(const float *__restrict__ mde, const float *__restrict__ disp,
                                                           const float *__restrict__ conf, int n, float q_lo,
                                                           float q_hi, float *__restrict__ scale,
                                                           float *__restrict__ shift, Rec... rec) {
  static_assert(sizeof...(Rec) == (STATS ? 1 : 0), "STATS takes the record pointer");
  __shared__ unsigned hist[L1_BINS];           // pass A (the fallback: its digit histograms)
  __shared__ unsigned pool[L1_POOL];           // the selected bins' keys
  __shared__ unsigned seg[L1_BINS / L1_SEG];   // 8-bin sums; then [4][512] digit histograms
  static_assert(L1_BINS / L1_SEG >= 4 * 512 && L1_BINS >= L1_POOL, "LDS reuse");
  __shared__ unsigned s_bin[4], s_rem[4], s_off[4], s_cnt[4], s_pre[4], s_total;
  __shared__ int s_list[4], s_fall;
  __shared__ double red[LSQ_THREADS / 64];
  __shared__ float qv[2];
  const int b = blockIdx.x;
  const float *md = mde + (long)b * n, *dd = disp + (long)b * n, *cd = conf + (long)b * n;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;

  // ranks of torch.quantile(linear): rank = q * (n - 1) in fp32
  const float r_lo = q_lo * (float)(n - 1), r_hi = q_hi * (float)(n - 1);
  if (t < 4) {
    const float r = (t < 2) ? r_lo : r_hi;
    s_rem[t] = (unsigned)((t & 1) ? ceilf(r) : truncf(r));
  }
  for (int i = t; i < L1_BINS; i += LSQ_THREADS) hist[i] = 0u;
  __syncthreads();
  // A: histogram of the top bits
  lsq_stream_keys(dd, n, [&](unsigned k, int, bool v) { hist_add(hist, bin_of(k), v); });
  __syncthreads();
  {
    unsigned sacc = 0;
#pragma unroll
    for (int k = 0; k < L1_SEG; ++k) sacc += hist[t * L1_SEG + k];
    for (int q = t + LSQ_THREADS; q < L1_BINS / L1_SEG; q += LSQ_THREADS) {   // (L1_BINS / L1_SEG > LSQ_THREADS)
      unsigned a2 = 0;
#pragma unroll
      for (int k = 0; k < L1_SEG; ++k) a2 += hist[q * L1_SEG + k];
      seg[q] = a2;
    }
    seg[t] = sacc;
  }
  __syncthreads();
  if (wv < 4) {   // wave r: rank r's bin and the keys below it
    int sg;
    unsigned below;
    wave_find<L1_BINS / L1_SEG / 64>(seg, s_rem[wv], sg, below);
    if (lane == 0) {
      unsigned acc = below, rem = s_rem[wv];
      int bin = sg * L1_SEG + L1_SEG - 1;
      for (int k = 0; k < L1_SEG; ++k) {
        const unsigned c = hist[sg * L1_SEG + k];
        if (acc + c > rem) {
          bin = sg * L1_SEG + k;
          break;
        }
        acc += c;
      }
      s_bin[wv] = (unsigned)bin;
      s_rem[wv] = rem - acc;   // the rank within its bin
    }
  }
  __syncthreads();
  if (t == 0) {   // pool slices of the distinct bins
    unsigned off = 0;
    int fall = 0;
    for (int r = 0; r < 4; ++r) {
      int src = r;
      for (int q = r - 1; q >= 0; --q)
        if (s_bin[q] == s_bin[r]) src = q;
      s_list[r] = src;
      if (src == r) {
        s_off[r] = off;
        s_cnt[r] = 0u;
        if (s_bin[r] != 0u) off += hist[s_bin[r]];   // (the zero bin is not pooled: its key is 0)
      }
    }
    fall = off > (unsigned)L1_POOL;
    s_fall = fall;
    s_total = off;
  }
  __syncthreads();
  const bool fall = s_fall != 0;
  unsigned lb[4];
  int lsrc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lb[r] = s_bin[r];
    lsrc[r] = s_list[r];
  }
  double s11 = 0, s12 = 0, s22 = 0, t1 = 0, t2 = 0;
  auto add_terms = [&](float d, float mv, float cv) __attribute__((always_inline)) {
    const float m = fabsf(mv);
    const float cc = fabsf(cv) * 0.9f + 0.1f;
    const float w = sqrtf(cc);
    const float a1 = m * w, y = fabsf(d) * w;
    s11 += (double)a1 * a1;
    s12 += (double)a1 * w;
    s22 += (double)w * w;
    t1 += (double)a1 * y;
    t2 += (double)w * y;
  };
  // the zero keys' terms (d = 0: no t1 / t2 part), kept apart until the band is known: they are
  // inside it iff the lower quantile is 0, possible only when the floor rank's bin is the zero bin
  double z11 = 0, z12 = 0, z22 = 0;
  const bool zero_lo = lb[0] == 0u;
  auto add_zero = [&](float mv, float cv) __attribute__((always_inline)) {
    const float m = fabsf(mv);
    const float w = sqrtf(fabsf(cv) * 0.9f + 0.1f);
    const float a1 = m * w;
    z11 += (double)a1 * a1;
    z12 += (double)a1 * w;
    z22 += (double)w * w;
  };
  unsigned long long sel_mask = 0ull;   // bit i: key i * LSQ_THREADS + t is in a selected (pooled) bin, i < 64
  if (!fall) {
    // B: copy the selected bins' keys into their pool slices (wave-aggregated appends) and mark them
    // in sel_mask; the normal equations of the keys strictly between the quantiles' bins
    const unsigned in_lo = lb[1], in_hi = lb[2];   // (b0 <= b1 <= b2 <= b3)
    auto append = [&](unsigned k, bool valid) __attribute__((always_inline)) {
      const unsigned bin = bin_of(k);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (lsrc[r] != r || lb[r] == 0u) continue;   // (uniform; the zero bin is not pooled)
        const bool hit = valid && bin == lb[r];
        const unsigned long long m = __ballot(hit);
        if (!m) continue;
        const int leader = __ffsll((long long)m) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(&s_cnt[r], (unsigned)__popcll(m));
        base = (unsigned)__builtin_amdgcn_readlane((int)base, leader);
        if (hit) {
          const unsigned at = s_off[r] + base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
          pool[at] = k;
        }
      }
    };
    for (int base = 0; base < n; base += 8 * LSQ_THREADS) {
      unsigned kv[8];
      float mv[8], cv[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {   // (clamped loads, all in flight together)
        const int jc = min(base + c * LSQ_THREADS + t, n - 1);
        kv[c] = key_of(dd[jc]);
        mv[c] = md[jc];
        cv[c] = cd[jc];
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int j = base + c * LSQ_THREADS + t;
        const unsigned bin = bin_of(kv[c]);
        append(kv[c], j < n);
        const int slot = base / LSQ_THREADS + c;
        if (slot < 64 && j < n && bin != 0u && (bin == lb[0] || bin == lb[1] || bin == lb[2] || bin == lb[3]))
          sel_mask |= 1ull << slot;
        if (j < n && bin > in_lo && bin < in_hi) add_terms(__uint_as_float(kv[c]), mv[c], cv[c]);
        if (zero_lo && j < n && bin == 0u) add_zero(mv[c], cv[c]);
      }
    }
    __syncthreads();
    // C: the low 17 bits of each rank's key as a 9-bit and an 8-bit digit (seg reused as [4][512])
    if (t < 4) s_pre[t] = lb[t] ? (lb[t] - 1u) << L1_SHIFT : 0u;   // (a zero-bin rank: key 0, done)
    for (int pass = 0; pass < 2; ++pass) {
      const int sh = pass == 0 ? 8 : 0, bits = pass == 0 ? 9 : 8;   // bits 16..8, then 7..0
      for (int i = t; i < 4 * 512; i += LSQ_THREADS) seg[i] = 0u;
      __syncthreads();
      unsigned pre[4];
      int src[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pre[r] = s_pre[r];
        src[r] = r;
        for (int q = r - 1; q >= 0; --q)   // (same bin too: a bin-1 rank's prefix is 0 like the zero bin's)
          if (pre[q] == pre[r] && lb[q] == lb[r]) src[r] = q;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (src[r] != r || lb[r] == 0u) continue;   // (uniform)
        const int L = lsrc[r];
        const unsigned cnt = s_cnt[L], off = s_off[L];
        for (unsigned e0 = 0; e0 < cnt; e0 += LSQ_THREADS) {
          const unsigned e = e0 + t;
          const unsigned k = e < cnt ? pool[off + e] : 0u;
          const bool match = e < cnt && (pass == 0 || ((k ^ pre[r]) >> (sh + bits)) == 0u);
          hist_add(seg + 512 * r, (k >> sh) & ((1u << bits) - 1u), match);
        }
      }
      __syncthreads();
      if (wv < 4 && pick4(lb, wv) != 0u) {
        int d;
        unsigned below;
        wave_find<8>(seg + 512 * pick4(src, wv), s_rem[wv], d, below);
        if (lane == 0) {
          s_rem[wv] -= below;
          s_pre[wv] = pick4(pre, wv) | ((unsigned)d << sh);
        }
      }
      __syncthreads();
    }
  } else {
    if (t < 4) {
      const float r = (t < 2) ? r_lo : r_hi;
      s_rem[t] = (unsigned)((t & 1) ? ceilf(r) : truncf(r));
    }
    __syncthreads();
    lsq_select_radix(dd, n, hist, s_pre, s_rem);
  }
  if (t < 2) {
    const float r = t == 0 ? r_lo : r_hi;
    const float lo = __uint_as_float(s_pre[2 * t]), hi = __uint_as_float(s_pre[2 * t + 1]);
    qv[t] = lerp_ref(lo, hi, r - truncf(r));
  }
  __syncthreads();
  const float qlo = qv[0], qhi = qv[1];
  if (!fall && zero_lo && qlo <= 0.0f) {   // the zeros are inside the band (d = 0 >= lo = 0)
    s11 += z11;
    s12 += z12;
    s22 += z22;
  }
  if (!fall) {
    // The boundary bins' keys inside the band, in index order: thread t takes j = t, t + 1024, ... as
    // in pass B, so which thread adds a term, and after which others, depends on the key's index and
    // value alone.  (Walking pool[] instead made both depend on where the waves' LDS appends of pass
    // B had put the key, that is on wave timing.)  Pass B marked which of the thread's first 64 keys
    // fell into a selected bin (sel_mask: the model's sample has 63.75 keys per thread), so only those
    // are loaded again; keys past that are streamed and tested.  Nothing to add when no key was pooled.
    if (s_total != 0u) {
      for (unsigned long long mk = sel_mask; mk; mk &= mk - 1ull) {   // this thread's marked keys, ascending
        const int j = (__ffsll((long long)mk) - 1) * LSQ_THREADS + t;
        const float d = __uint_as_float(key_of(dd[j]));
        if (qlo <= d && d <= qhi) add_terms(d, md[j], cd[j]);
      }
      if (n > 64 * LSQ_THREADS) {   // (past 64 keys per thread nothing was marked: test every key)
        const int off = 64 * LSQ_THREADS;
        lsq_stream_keys(dd + off, n - off, [&](unsigned k, int j, bool valid) {
          const unsigned bin = bin_of(k);
          const float d = __uint_as_float(k);
          if (valid && bin != 0u && (bin == lb[0] || bin == lb[1] || bin == lb[2] || bin == lb[3]) && qlo <= d &&
              d <= qhi)
            add_terms(d, md[off + j], cd[off + j]);
        });
      }
    }
  } else {   // (the fallback: every key against the band)
    for (int base = 0; base < n; base += 8 * LSQ_THREADS) {
      float dv[8], mv[8], cv[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int j = base + c * LSQ_THREADS + t, jc = min(j, n - 1);
        dv[c] = __uint_as_float(key_of(dd[jc]));
        if (j >= n) dv[c] = -1.0f;   // (outside every band)
        mv[c] = md[jc];
        cv[c] = cd[jc];
      }
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (qlo <= dv[c] && dv[c] <= qhi) add_terms(dv[c], mv[c], cv[c]);
    }
  }
  s11 = block_sum(s11, red);
  s12 = block_sum(s12, red);
  s22 = block_sum(s22, red);
  t1 = block_sum(t1, red);
  t2 = block_sum(t2, red);
  if (t == 0) {
    const double det = s11 * s22 - s12 * s12;
    double sc, sh;
    if (s22 > 0 && fabs(det) > 1e-12 * s11 * s22) {
      sc = (s22 * t1 - s12 * t2) / det;
      sh = (s11 * t2 - s12 * t1) / det;
    } else if (s22 > 0) {
      // rank-deficient (all kept mono values equal): minimum-norm solution like gelsy
      const double m0 = s12 / s22, c0 = t2 / s22;
      sc = c0 * m0 / (m0 * m0 + 1.0);
      sh = c0 / (m0 * m0 + 1.0);
    } else {
      sc = 0.0;
      sh = 0.0;
    }
    scale[b] = (float)sc;
    shift[b] = (float)sh;
    if constexpr (STATS) {
      double *r = (rec, ...) + (long)b * SA_LSQ_REC;
      r[0] = s11;
      r[1] = s12;
      r[2] = s22;
      r[3] = (double)qlo;
      r[4] = (double)qhi;
      r[5] = !(s22 > 0) ? 2.0 : !(fabs(det) > 1e-12 * s11 * s22) ? 1.0 : 0.0;
    }
  }
}

}  // namespace

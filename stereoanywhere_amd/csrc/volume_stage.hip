// The volume stage of the fine-tuning forward: the volume-corruption augmentations
// (stereoanywhere.py:214-251) and the truncation multiply (201-205, 253-254, utils.py:216-238) on an
// existing [B,1,H,W1,W2] volume, one pass, plus the device-side maximum the "zeroing" branches scale
// their Gaussian with (torch.max(volume).cpu().item() in the reference: a host sync).
//
// All three kernels are memory-bound streams (one volume read, one written, a few per-row scalars).
// Layout: a wave owns whole rows (b, h, j) of W2 floats, ROWS_PER_WAVE of them back to back; a lane
// moves 16 bytes along k per step (dword-aligned vector accesses: a row of a volume with W2 % 4 != 0
// does not start on a 16-byte boundary), lanes 0..2 finish the W2 % 4 tail with dwords.  The row's
// own terms (its mask bit, noise factor, truncation disparity and confidence, the rolled source row)
// are wave-uniform and are loaded once per row.  A rolled row is another row of the same slice read
// whole, so it stays one coalesced read.
//
// The reference writes the blend v (1 - m) + src m with m in {0, 1}; this pass writes the selected
// value, which is the same number for finite volumes.
#include "sa_common.h"
#include "volume_common.h"

namespace {

// 16 bytes at dword alignment (global loads and stores of gfx950 need no more)
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

constexpr int ROWS_PER_WAVE = 4;
constexpr int WAVES = 4;
constexpr int PEAK_MAX_PARTS = 1024;

template <int KIND, bool TRUNC>
__global__ __launch_bounds__(64 * WAVES) void volume_stage_kernel(
    const float *vol, long rows, int W1, int W2, const float *__restrict__ mde, int nbins, int bin, int shift,
    const float *__restrict__ noise, const float *__restrict__ peak, const float *__restrict__ tdisp,
    const float *__restrict__ tconf, float atten, float *out) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const long row0 = ((long)blockIdx.x * WAVES + wave) * ROWS_PER_WAVE;
  const int nvec = W2 >> 2;
  for (int r = 0; r < ROWS_PER_WAVE; ++r) {
    const long row = row0 + r;
    if (row >= rows) break;
    const int j = (int)(row % W1);
    bool m = false;
    if (KIND != SA_VOLAUG_NONE) m = sa::depth_bin(mde[row], nbins) == bin;
    long src = row;
    float scale = 1.0f, d = 0.0f, t = 0.0f;
    if (KIND == SA_VOLAUG_ROLL && m) {
      int js = j - shift;   // shift in 1..W1
      if (js < 0) js += W1;
      src = row - j + js;
    }
    if (KIND == SA_VOLAUG_NOISE && m) scale = noise[row];
    if (KIND == SA_VOLAUG_ZERO && m) scale = peak[0];
    if (TRUNC) {
      d = tdisp[row];
      t = tconf[row];
    }
    auto cell = [&](float v, int k) __attribute__((always_inline)) {
      float c = v;
      if (KIND == SA_VOLAUG_NOISE && m) c = v * scale;
      if (KIND == SA_VOLAUG_ZERO && m) {   // gauss_corr_volume_naive(zeros, gauss_k = peak): the curve first
        const float x = (float)j - (float)k;
        c = v * (scale * expf(-(x * x) / 2.0f));
      }
      if (TRUNC) c = sa::trunc_factor<false>(j, k, d, t, atten) * c;
      return c;
    };
    const float *in = vol + src * W2;
    float *o = out + row * W2;
    for (int q = lane; q < nvec; q += 64) {
      const f32x4u v = *reinterpret_cast<const f32x4u *>(in + 4 * q);
      f32x4u w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = cell(v[e], 4 * q + e);
      *reinterpret_cast<f32x4u *>(o + 4 * q) = w;
    }
    const int kt = 4 * nvec + lane;
    if (kt < W2) o[kt] = cell(in[kt], kt);
  }
}

// (max, NaN seen) of a block's values -> thread 0; torch.max gives NaN when any element is one,
// fmaxf drops them, so the flag travels beside the maximum
__device__ __forceinline__ void block_peak(float &mx, float &nan) {
  __shared__ float part[2][WAVES];
  float v[2] = {mx, nan};
  sa::wave_max_dpp_n<2>(v);
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = v[0];
    part[1][threadIdx.x >> 6] = v[1];
  }
  __syncthreads();
  mx = part[0][0];
  nan = part[1][0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) {
    mx = fmaxf(mx, part[0][w]);
    nan = fmaxf(nan, part[1][w]);
  }
}

__device__ __forceinline__ void peak_take(float x, float &mx, float &nan) {
  if (x != x) nan = 1.0f;
  mx = fmaxf(mx, x);
}

// stage 1: block b's maximum of its grid-strided share -> work[b] (NaN when it saw one)
__global__ __launch_bounds__(64 * WAVES) void volume_peak_partial_kernel(const float *__restrict__ v, long count,
                                                                         float *__restrict__ work) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const long nvec = count >> 2;
  float mx = -INFINITY, nan = 0.0f;
  for (long q = tid; q < nvec; q += stride) {
    const f32x4u x = *reinterpret_cast<const f32x4u *>(v + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) peak_take(x[e], mx, nan);
  }
  for (long i = 4 * nvec + tid; i < count; i += stride) peak_take(v[i], mx, nan);
  block_peak(mx, nan);
  if (threadIdx.x == 0) work[blockIdx.x] = nan != 0.0f ? __builtin_nanf("") : mx;
}

// stage 2: one block folds the partials
__global__ __launch_bounds__(64 * WAVES) void volume_peak_final_kernel(const float *__restrict__ work, int parts,
                                                                       float *__restrict__ peak) {
  float mx = -INFINITY, nan = 0.0f;
  for (int i = threadIdx.x; i < parts; i += blockDim.x) peak_take(work[i], mx, nan);
  block_peak(mx, nan);
  if (threadIdx.x == 0) peak[0] = nan != 0.0f ? __builtin_nanf("") : mx;
}

bool overlap(const float *a, const float *b, long n) { return a < b + n && b < a + n; }

template <int KIND>
void launch_stage(bool trunc, unsigned grid, hipStream_t s, const float *vol, long rows, int W1, int W2,
                  const float *mde, int nbins, int bin, int shift, const float *noise, const float *peak,
                  const float *tdisp, const float *tconf, float atten, float *out) {
  if (trunc) {
    volume_stage_kernel<KIND, true><<<grid, 64 * WAVES, 0, s>>>(vol, rows, W1, W2, mde, nbins, bin, shift, noise, peak,
                                                                tdisp, tconf, atten, out);
  } else {
    volume_stage_kernel<KIND, false><<<grid, 64 * WAVES, 0, s>>>(vol, rows, W1, W2, mde, nbins, bin, shift, noise, peak,
                                                                 tdisp, tconf, atten, out);
  }
}

}  // namespace

extern "C" int sa_volume_peak(const float *volume, long count, float *peak, float *work, long work_floats,
                              void *stream) {
  SA_REQUIRE(volume && peak && work, "sa_volume_peak: null pointer (volume / peak / work)");
  SA_REQUIRE(count > 0, "sa_volume_peak: count must be positive (got %ld)", count);
  SA_REQUIRE(work_floats > 0, "sa_volume_peak: work_floats must be positive (got %ld)", work_floats);
  // a block per 4096 floats (256 lanes x 16 bytes x 4 steps), as many as the workspace holds
  long parts = (count + 4095) / 4096;
  if (parts > work_floats) parts = work_floats;
  if (parts > PEAK_MAX_PARTS) parts = PEAK_MAX_PARTS;
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  volume_peak_partial_kernel<<<(unsigned)parts, 64 * WAVES, 0, s>>>(volume, count, work);
  volume_peak_final_kernel<<<1, 64 * WAVES, 0, s>>>(work, (int)parts, peak);
  return sa::check_launch("sa_volume_peak");
}

extern "C" int sa_volume_stage(const float *volume, int B, int H, int W1, int W2, int kind, const float *mde,
                               int nbins, int bin, int shift, const float *noise, const float *peak,
                               const float *trunc_disp, const float *trunc_conf, float atten, float *out,
                               void *stream) {
  SA_REQUIRE(volume && out, "sa_volume_stage: null pointer (volume / out)");
  SA_REQUIRE(B > 0 && H > 0 && W1 > 0 && W2 > 0, "sa_volume_stage: bad shape B %d H %d W1 %d W2 %d", B, H, W1, W2);
  const long rows = (long)B * H * W1;
  SA_REQUIRE(rows <= 0x7fffffffL, "sa_volume_stage: bad shape (B*H*W1 = %ld rows exceed 2^31 - 1)", rows);
  SA_REQUIRE(kind == SA_VOLAUG_NONE || kind == SA_VOLAUG_ROLL || kind == SA_VOLAUG_NOISE || kind == SA_VOLAUG_ZERO,
             "sa_volume_stage: kind must be SA_VOLAUG_NONE, _ROLL, _NOISE or _ZERO (got %d)", kind);
  SA_REQUIRE((trunc_disp == nullptr) == (trunc_conf == nullptr),
             "sa_volume_stage: trunc_disp and trunc_conf go together");
  if (kind != SA_VOLAUG_NONE) {
    SA_REQUIRE(mde, "sa_volume_stage: null pointer (mde, needed by every augmentation)");
    SA_REQUIRE(nbins >= 1 && nbins <= 64, "sa_volume_stage: nbins must be 1..64 (got %d)", nbins);
    SA_REQUIRE(bin >= 0 && bin < nbins, "sa_volume_stage: bin must be 0..nbins-1 (got %d of %d)", bin, nbins);
  }
  if (kind == SA_VOLAUG_ROLL) {
    SA_REQUIRE(shift >= 1 && shift <= W1, "sa_volume_stage: shift must be 1..W1 (got %d, W1 %d)", shift, W1);
    SA_REQUIRE(!overlap(volume, out, rows * W2), "sa_volume_stage: SA_VOLAUG_ROLL cannot run in place (out overlaps volume)");
  }
  if (kind == SA_VOLAUG_NOISE) SA_REQUIRE(noise, "sa_volume_stage: null pointer (noise, needed by SA_VOLAUG_NOISE)");
  if (kind == SA_VOLAUG_ZERO) {
    SA_REQUIRE(peak, "sa_volume_stage: null pointer (peak, needed by SA_VOLAUG_ZERO)");
    SA_REQUIRE(W1 == W2, "sa_volume_stage: SA_VOLAUG_ZERO needs W1 == W2 (got %d and %d)", W1, W2);
  }
  const bool trunc = trunc_disp != nullptr;
  if (trunc) SA_REQUIRE(W1 == W2, "sa_volume_stage: the truncation needs W1 == W2 (got %d and %d)", W1, W2);
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  const unsigned grid = (unsigned)((rows + WAVES * ROWS_PER_WAVE - 1) / (WAVES * ROWS_PER_WAVE));
#define SA_STAGE(K_) \
  launch_stage<K_>(trunc, grid, s, volume, rows, W1, W2, mde, nbins, bin, shift, noise, peak, trunc_disp, trunc_conf, atten, out)
  switch (kind) {
    case SA_VOLAUG_ROLL: SA_STAGE(SA_VOLAUG_ROLL); break;
    case SA_VOLAUG_NOISE: SA_STAGE(SA_VOLAUG_NOISE); break;
    case SA_VOLAUG_ZERO: SA_STAGE(SA_VOLAUG_ZERO); break;
    default: SA_STAGE(SA_VOLAUG_NONE); break;
  }
#undef SA_STAGE
  return sa::check_launch("sa_volume_stage");
}

extern "C" int sa_volume_truncate_backward(const float *grad_out, int B, int H, int W1, int W2,
                                           const float *trunc_disp, const float *trunc_conf, float atten,
                                           float *grad_volume, void *stream) {
  SA_REQUIRE(grad_out && trunc_disp && trunc_conf && grad_volume,
             "sa_volume_truncate_backward: null pointer (grad_out / trunc_disp / trunc_conf / grad_volume)");
  SA_REQUIRE(B > 0 && H > 0 && W1 > 0 && W2 > 0, "sa_volume_truncate_backward: bad shape B %d H %d W1 %d W2 %d", B, H,
             W1, W2);
  const long rows = (long)B * H * W1;
  SA_REQUIRE(rows <= 0x7fffffffL, "sa_volume_truncate_backward: bad shape (B*H*W1 = %ld rows exceed 2^31 - 1)", rows);
  SA_REQUIRE(W1 == W2, "sa_volume_truncate_backward: the truncation needs W1 == W2 (got %d and %d)", W1, W2);
  // the factor does not depend on the volume: the adjoint of v -> factor v is the forward's own
  // kernel on the upstream gradient (the same instantiation, so the same per-cell arithmetic)
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_MISC, s);
  const unsigned grid = (unsigned)((rows + WAVES * ROWS_PER_WAVE - 1) / (WAVES * ROWS_PER_WAVE));
  volume_stage_kernel<SA_VOLAUG_NONE, true><<<grid, 64 * WAVES, 0, s>>>(grad_out, rows, W1, W2, nullptr, 0, 0, 0, nullptr,
                                                                       nullptr, trunc_disp, trunc_conf, atten,
                                                                       grad_volume);
  return sa::check_launch("sa_volume_truncate_backward");
}

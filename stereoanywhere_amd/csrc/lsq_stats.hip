// sa_weighted_lsq_stats: the forward of the differentiable weighted_lsq.  The second instance of
// lsq1_kernel (lsq_select.h): the same selection, sums and solve as sa_weighted_lsq, so the same
// scale and shift bits, plus the per-sample record sa_weighted_lsq_backward (lsq_backward.hip) reads.
// A file of its own so that lsq.hip, with the one instance it always had, compiles to the code it
// always did.
#include <cstdint>

#include "lsq_select.h"
#include "sa_common.h"

extern "C" int sa_weighted_lsq_stats(const float *mde, const float *disp, const float *conf, int B, int n_per_b,
                                     float q_lo, float q_hi, float *scale, float *shift, double *rec,
                                     void *stream) {
  SA_REQUIRE(mde && disp && conf && scale && shift && rec, "sa_weighted_lsq_stats: null pointer");
  SA_REQUIRE(B > 0 && n_per_b > 0, "sa_weighted_lsq_stats: empty input");
  SA_REQUIRE(q_lo >= 0.f && q_lo <= q_hi && q_hi <= 1.f, "sa_weighted_lsq_stats: quantiles out of order");
  SA_REQUIRE((reinterpret_cast<uintptr_t>(rec) & 7) == 0, "sa_weighted_lsq_stats: record not 8-byte aligned");
  hipStream_t s = sa::as_stream(stream);
  sa::TimingScope ts(SA_K_LSQ, s);
  lsq1_kernel<true><<<B, LSQ_THREADS, 0, s>>>(mde, disp, conf, n_per_b, q_lo, q_hi, scale, shift, rec);
  return sa::check_launch("sa_weighted_lsq_stats");
}

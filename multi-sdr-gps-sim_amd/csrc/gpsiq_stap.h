// gpsiq_stap.h -- what the device context holds for gpsiq_stap_cov / gpsiq_stap_combine (include/gpsiq_rows.h, "Space-time array") and
// what their host side (gpsiq_stap.cpp) and their kernels (gpsiq_stap_kernels.hip, with gpsiq_stap_geometry.h) use of each other.  The
// plan is in gpsiq_stap_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `stap`.
#ifndef GPSIQ_STAP_H
#define GPSIQ_STAP_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"
#include "gpsiq_stage_call.h"
#include "gpsiq_stap_geometry.h"

namespace gpsiq {

static_assert(kStapMaxElem == GPSIQ_ARRAY_MAX_ELEM && kStapMaxTaps == GPSIQ_STAP_MAX_TAPS && kStapMaxRows == GPSIQ_STAP_MAX_ROWS,
              "the geometry's sizes are the contract's");

// the streams, their heads and the weights of a call as the kernels take them: by value, in the argument block, wave-uniform
struct StapSources { const uint8_t *p[kStapMaxElem]; const uint8_t *head[kStapMaxElem]; };      // head[e] null: zeros before the span
struct StapWeights { uint32_t w[kStapMaxRows]; };                      // row e T + t: re in the low half, im in the high half

// the covariance kernels' scratch (the real Gram matrix, or R itself: gpsiq_stap_plan.h) on the device and page-locked on its way
// back; the combiner's counter with the two events either call is timed with
struct StapSet {
    DevBuf<unsigned long long>    d_gram;   PinnedBuf<unsigned long long> h_gram;     // [kStapGramWords]
    ClipCount      clip;
    long           last[5] = {-1, 0, 0, 0, 0};      // the last call's plan: kernel, grid, run, elements, taps (gpsiq_stap_last_plan)
    int reserve();                                  // first use
};

inline int StapSet::reserve()
{
    if (int rc = clip.reserve()) return rc;
    HIP_TRY(reserve_together(kStapGramWords, kStapGramWords, d_gram, h_gram));
    return GPSIQ_OK;
}

// the stage's kernels (gpsiq_stap_kernels.hip).  Generic covariance: streams and heads, elements, taps, samples, runs of the span,
// scratch.  Matrix covariance: streams and heads, elements, taps, samples, k-steps of the span and of a run, scratch.  Combiner:
// streams and heads, weights, elements, taps, samples, shift, destination, lead, slots, the counter of clamped elements
// (gpsiq_stap_plan.h)
using StapCovFn     = void (*)(const StapSources, int, int, int, uint64_t, unsigned long long *);
using StapCovMfmaFn = void (*)(const StapSources, int, int, int, uint64_t, uint64_t, unsigned long long *);
using StapCombineFn = void (*)(const StapSources, const StapWeights, int, int, int, int, uint8_t *, int, uint64_t, unsigned long long *);
StapCovFn     stap_cov_generic_kernel(int fmt);
StapCovMfmaFn stap_cov_mfma_kernel(int fmt, int groups);
StapCombineFn stap_combine_kernel(int in_fmt, int out_fmt);

}  // namespace gpsiq

// gpsiq_stap.cpp: the two calls themselves, behind the plumbing entries "stap_cov" and "stap_combine".  Declared from the public
// prototypes, and hidden: a definition that has drifted from include/gpsiq_rows.h is another function, and the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_stap_cov) gpsiq_stap_cov_impl;
__attribute__((visibility("hidden"))) decltype(gpsiq_stap_combine) gpsiq_stap_combine_impl;
#endif

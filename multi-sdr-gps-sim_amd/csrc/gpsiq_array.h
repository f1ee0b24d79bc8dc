// gpsiq_array.h -- what the device context holds for gpsiq_array_cov / gpsiq_array_combine (include/gpsiq_rows.h, "Array") and what
// their host side (gpsiq_array.cpp) and their kernels (gpsiq_array_kernels.hip, with gpsiq_array_geometry.h) use of each other.  The
// plan is in gpsiq_array_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `array`.
#ifndef GPSIQ_ARRAY_H
#define GPSIQ_ARRAY_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"
#include "gpsiq_stage_call.h"
#include "gpsiq_array_geometry.h"

namespace gpsiq {

static_assert(kArrMaxElem == GPSIQ_ARRAY_MAX_ELEM, "the geometry's element count is the contract's");

// the streams and the weights of a call as the kernels take them: by value, so they sit in argument registers, wave-uniform
struct ArraySources { const uint8_t *p[kArrMaxElem]; };
struct ArrayWeights { uint32_t w[kArrMaxElem]; };                      // re in the low half, im in the high half

// the covariance kernels' scratch (the Gram tile, or R itself: gpsiq_array_plan.h) on the device and page-locked on its way back;
// the combiner's counter with the two events either call is timed with
struct ArraySet {
    DevBuf<unsigned long long>    d_gram;   PinnedBuf<unsigned long long> h_gram;     // [kArrGramWords]
    ClipCount      clip;
    long           last[4] = {-1, 0, 0, 0};         // the last call's plan: kernel, grid, run, elements (gpsiq_array_last_plan)
    int reserve();                                  // first use
};

inline int ArraySet::reserve()
{
    if (int rc = clip.reserve()) return rc;
    HIP_TRY(reserve_together(kArrGramWords, kArrGramWords, d_gram, h_gram));
    return GPSIQ_OK;
}

// the stage's kernels (gpsiq_array_kernels.hip).  Generic covariance: streams, elements, samples, runs of the span, scratch.
// Matrix covariance: streams, elements, samples, k-steps of the span and of a run, scratch.  Combiner: streams, weights, elements,
// samples, shift, destination, lead, slots, the counter of clamped elements (gpsiq_array_plan.h)
using ArrayCovFn     = void (*)(const ArraySources, int, int, uint64_t, unsigned long long *);
using ArrayCovMfmaFn = void (*)(const ArraySources, int, int, uint64_t, uint64_t, unsigned long long *);
using ArrayCombineFn = void (*)(const ArraySources, const ArrayWeights, int, int, int, uint8_t *, int, uint64_t, unsigned long long *);
ArrayCovFn     array_cov_generic_kernel(int fmt);
ArrayCovMfmaFn array_cov_mfma_kernel(int fmt);
ArrayCombineFn array_combine_kernel(int in_fmt, int out_fmt);

}  // namespace gpsiq

// gpsiq_array.cpp: the two calls themselves, behind the plumbing entries "array_cov" and "array_combine".  Declared from the public
// prototypes, and hidden: a definition that has drifted from include/gpsiq_rows.h is another function, and the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_array_cov) gpsiq_array_cov_impl;
__attribute__((visibility("hidden"))) decltype(gpsiq_array_combine) gpsiq_array_combine_impl;
#endif

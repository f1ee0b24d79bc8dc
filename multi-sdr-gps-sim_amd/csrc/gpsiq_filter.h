// gpsiq_filter.h -- what the device context holds for gpsiq_filter / gpsiq_generate_batch_filtered (include/gpsiq_rows.h, "Filter") and
// what their host side (gpsiq_filter.cpp) and their kernels (gpsiq_filter_kernels.hip, with gpsiq_filter_geometry.h) use of each
// other.  The plan is in gpsiq_filter_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `filt`.
#ifndef GPSIQ_FILTER_H
#define GPSIQ_FILTER_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"
#include "gpsiq_filter_geometry.h"

namespace gpsiq {

// the coefficients of a call on the device and page-locked on their way there (the taps as dwords, then the matrix kernel's digit
// planes: one size, the largest a call can ask for), the counter of clamped elements and its page-locked twin, and the two events a
// kernel is timed with.  The batch call works through its pieces with the context's staging ring (gpsiq_stage_batch.h)
struct FilterSet {
    static constexpr size_t kTapBytes = 4 * (size_t) kFiltMaxTaps;
    static constexpr size_t kCoefBytes = kTapBytes + (size_t) filter_mfma_plane_bytes(kFiltMaxSteps);
    DevBuf<uint8_t>               d_coef;    PinnedBuf<uint8_t>            h_coef;        // [kCoefBytes]
    DevBuf<unsigned long long>    d_count;   PinnedBuf<unsigned long long> h_count;       // [1]
    Event          t0, t1;
    long           last[4] = {-1, 0, 0, 0};         // the last call's plan: kernel, grid, outputs per run, pieces (gpsiq_filter_last_plan)
    int reserve();                                  // first use
};

inline int FilterSet::reserve()
{
    HIP_TRY(t0.ensure(hipEventDefault));
    HIP_TRY(t1.ensure(hipEventDefault));
    HIP_TRY(reserve_together(kCoefBytes, kCoefBytes, d_coef, h_coef));
    HIP_TRY(d_count.reserve(1));
    HIP_TRY(h_count.reserve(1));
    return GPSIQ_OK;
}

// the filter kernels (gpsiq_filter_kernels.hip).  Arguments: span and its samples, head, the taps as dwords (generic) or the digit
// planes (matrix), ntaps, shift, decim, phase, destination, outputs of the span, outputs of a run, runs of the launch
// (gpsiq_filter_plan.h); matrix kernel: the k-steps of a tile; the counter of clamped elements
using FilterGenericFn = void (*)(const uint8_t *, int, const uint8_t *, const int32_t *, int, int, int, int, uint8_t *, int, int, uint64_t,
                                 unsigned long long *);
using FilterMfmaFn    = void (*)(const uint8_t *, int, const uint8_t *, const uint8_t *, int, int, int, int, uint8_t *, int, int, uint64_t, int,
                                 unsigned long long *);
FilterGenericFn filter_generic_kernel(int in_fmt, int out_fmt);
FilterMfmaFn    filter_mfma_kernel(int out_fmt);

}  // namespace gpsiq

// gpsiq_filter.cpp: gpsiq_filter and gpsiq_generate_batch_filtered themselves, behind the plumbing entries "filter" and
// "generate_batch_filtered".  Declared from the public prototypes, and hidden: a definition that has drifted from
// include/gpsiq_rows.h is another function, and the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_filter) gpsiq_filter_impl;
__attribute__((visibility("hidden"))) decltype(gpsiq_generate_batch_filtered) gpsiq_generate_batch_filtered_impl;
#endif

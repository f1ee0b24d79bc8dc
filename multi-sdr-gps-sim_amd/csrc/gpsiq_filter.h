// gpsiq_filter.h -- what the device context holds for gpsiq_filter / gpsiq_generate_batch_filtered (include/gpsiq_rows.h, "Filter") and
// what their host side (gpsiq_filter.cpp) and their kernels (gpsiq_filter_kernels.hip, with gpsiq_filter_geometry.h) use of each
// other.  The plan is in gpsiq_filter_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's members `filt`
// and `cfilt` (gpsiq_cfilter.h has the complex filter's kernel types).
#ifndef GPSIQ_FILTER_H
#define GPSIQ_FILTER_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"
#include "gpsiq_stage_call.h"
#include "gpsiq_filter_geometry.h"

namespace gpsiq {

// What a FIR stage keeps in the context: gpsiq_filter's set (`filt`) and gpsiq_cfilter's (`cfilt`), one each.  The coefficients of
// a call on the device and page-locked on their way there (the taps as dwords -- complex ones re below and im above -- then the
// matrix kernels' digit planes: one size, the largest a call can ask for), and the counter of clamped elements with its timing events
// (gpsiq_stage_call.h).  The batch call works through its pieces with the context's staging ring (gpsiq_stage_batch.h)
struct FirSet {
    static constexpr size_t kTapBytes = 4 * (size_t) kFiltMaxTaps;
    static constexpr size_t kCoefBytes = kTapBytes + (size_t) filter_mfma_plane_bytes(kFiltMaxSteps);
    DevBuf<uint8_t>               d_coef;    PinnedBuf<uint8_t>            h_coef;        // [kCoefBytes]
    ClipCount      clip;
    // the last call's plan: kernel, grid, outputs per run, then pieces (gpsiq_filter_last_plan) or k-steps (gpsiq_cfilter_last_plan)
    long           last[4] = {-1, 0, 0, 0};
    int reserve();                                  // first use
};

inline int FirSet::reserve()
{
    if (int rc = clip.reserve()) return rc;
    HIP_TRY(reserve_together(kCoefBytes, kCoefBytes, d_coef, h_coef));
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

// gpsiq_cfilter.h -- what the device context holds for gpsiq_cfilter (include/gpsiq_rows.h, "Complex filter and notch") and what its
// host side (gpsiq_cfilter.cpp) and its kernels (gpsiq_cfilter_kernels.hip, with gpsiq_cfilter_geometry.h) use of each other.  The plan
// is in gpsiq_cfilter_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `cfilt`.
#ifndef GPSIQ_CFILTER_H
#define GPSIQ_CFILTER_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"
#include "gpsiq_cfilter_geometry.h"

namespace gpsiq {

// the stage's own coefficients on the device and page-locked on their way there (the taps as dwords, re below and im above, then the
// matrix kernels' digit planes: one size, the largest a call can ask for), its own counter of clamped elements with its page-locked
// twin, and the two events a kernel is timed with: nothing is shared with gpsiq_filter's set
struct CfilterSet {
    static constexpr size_t kTapBytes = 4 * (size_t) kFiltMaxTaps;
    static constexpr size_t kCoefBytes = kTapBytes + (size_t) filter_mfma_plane_bytes(kFiltMaxSteps);
    DevBuf<uint8_t>               d_coef;    PinnedBuf<uint8_t>            h_coef;        // [kCoefBytes]
    DevBuf<unsigned long long>    d_count;   PinnedBuf<unsigned long long> h_count;       // [1]
    Event          t0, t1;
    long           last[4] = {-1, 0, 0, 0};         // the last call's plan: kernel, grid, outputs per run, k-steps (gpsiq_cfilter_last_plan)
    int reserve();                                  // first use
};

inline int CfilterSet::reserve()
{
    HIP_TRY(t0.ensure(hipEventDefault));
    HIP_TRY(t1.ensure(hipEventDefault));
    HIP_TRY(reserve_together(kCoefBytes, kCoefBytes, d_coef, h_coef));
    HIP_TRY(d_count.reserve(1));
    HIP_TRY(h_count.reserve(1));
    return GPSIQ_OK;
}

// the stage's kernels (gpsiq_cfilter_kernels.hip).  Arguments: span and its samples, head, the taps as dwords (generic) or the digit
// planes (matrix), ntaps, shift, decim, phase, destination, outputs of the span, outputs of a run, runs of the launch
// (gpsiq_cfilter_plan.h); matrix kernel: the k-steps of a tile and the two row constants; the counter of clamped elements.
// An int8 input's matrix kernel is filter_mfma (gpsiq_filter.h: FilterMfmaFn, filter_mfma_kernel)
using CfilterGenericFn = void (*)(const uint8_t *, int, const uint8_t *, const uint32_t *, int, int, int, int, uint8_t *, int, int, uint64_t,
                                  unsigned long long *);
using CfilterMfma16Fn  = void (*)(const uint8_t *, int, const uint8_t *, const uint8_t *, int, int, int, int, uint8_t *, int, int, uint64_t, int,
                                  int, int, unsigned long long *);
CfilterGenericFn cfilter_generic_kernel(int in_fmt, int out_fmt);
CfilterMfma16Fn  cfilter_mfma16_kernel(int out_fmt);

}  // namespace gpsiq

// gpsiq_cfilter.cpp: gpsiq_cfilter itself, behind the plumbing entry "cfilter".  Declared from the public prototype, and hidden: a
// definition that has drifted from include/gpsiq_rows.h is another function, and the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_cfilter) gpsiq_cfilter_impl;
#endif

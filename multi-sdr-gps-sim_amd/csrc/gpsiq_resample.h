// gpsiq_resample.h -- what the device context holds for gpsiq_resample / gpsiq_generate_batch_resampled (include/gpsiq_rows.h,
// "Resample") and what their host side (gpsiq_resample.cpp) and their kernels (gpsiq_resample_kernels.hip, with
// gpsiq_resample_geometry.h) use of each other.  The plan is in gpsiq_resample_plan.h.  Host code; gpsiq_ctx.h includes this header for
// the context's member `rs`.
#ifndef GPSIQ_RESAMPLE_H
#define GPSIQ_RESAMPLE_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"
#include "gpsiq_stage_call.h"
#include "gpsiq_resample_geometry.h"

namespace gpsiq {

// the tap table of a call on the device and page-locked on its way there (one size, the largest a call can ask for), and the counter
// of clamped elements with its timing events (gpsiq_stage_call.h).  The batch call works through its pieces with the context's
// staging ring (gpsiq_stage_batch.h)
struct ResampleSet {
    static constexpr size_t kTableEntries = (size_t) kRsMaxTable;
    DevBuf<int16_t>               d_taps;    PinnedBuf<int16_t>            h_taps;        // [kTableEntries]
    ClipCount      clip;
    long long      last[4] = {-1, 0, 0, 0};         // the last call's plan: kernel, grid, outputs per unit, pieces (gpsiq_resample_last_plan)
    int reserve();                                  // first use
};

inline int ResampleSet::reserve()
{
    if (int rc = clip.reserve()) return rc;
    HIP_TRY(reserve_together(kTableEntries, kTableEntries, d_taps, h_taps));
    return GPSIQ_OK;
}

// the resampler kernels (gpsiq_resample_kernels.hip).  Arguments: span and its samples, head, the device table int16
// [nphases + 1][ntaps], log2 of the phases, ntaps, shift, interp, step, pos0, destination, outputs of the span, (row kernel: outputs
// of a run,) units of the launch (gpsiq_resample_plan.h), the counter of clamped elements
using ResampleGenericFn = void (*)(const uint8_t *, int, const uint8_t *, const int16_t *, int, int, int, int, uint64_t, uint64_t, uint8_t *, uint64_t,
                                   uint64_t, unsigned long long *);
using ResampleRowsFn    = void (*)(const uint8_t *, int, const uint8_t *, const int16_t *, int, int, int, int, uint64_t, uint64_t, uint8_t *, uint64_t, int,
                                   uint64_t, unsigned long long *);
ResampleGenericFn resample_generic_kernel(int in_fmt, int out_fmt);
ResampleRowsFn    resample_rows_kernel(int in_fmt, int out_fmt, bool pad);

}  // namespace gpsiq

// gpsiq_resample.cpp: gpsiq_resample and gpsiq_generate_batch_resampled themselves, behind the plumbing entries "resample" and
// "generate_batch_resampled".  Declared from the public prototypes, and hidden: a definition that has drifted from
// include/gpsiq_rows.h is another function, and the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_resample) gpsiq_resample_impl;
__attribute__((visibility("hidden"))) decltype(gpsiq_generate_batch_resampled) gpsiq_generate_batch_resampled_impl;
#endif
